"""GPU tests (-m gpu) of the decoder on streams our encoder never writes: P-frames from a multi-worker reference (the oracle's
seeded emulation of DecideBlockTypes' thread race, OracleCodec.set_p_race), key frames cut into 5..32 uneven worker bands,
and frames of exactly k * 131072 coder entries, which end without a tail block (tests/foreign_streams.py).  Every picture
is checked against the oracle's decoder and against the input (the streams are lossless)."""
import numpy as np
import pytest

import foreign_streams as foreign
import oracle_api as O
from screenpressor_amd.synth import DesktopSequence, pack24

pytestmark = pytest.mark.gpu


def _codec(w, h, bpp=32, **kw):
    from screenpressor_amd.codec import ScreenCodec
    return ScreenCodec(0).Init(w, h, bpp, **kw)


def _dev(packets):
    import torch
    data = b"".join(packets)
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()  # exactly the packets' bytes, no slack


class Stream:
    """packets of one oracle-encoded stream, the input rows and the oracle's decoded rows"""

    def __init__(self, frames, bpp=32, race=(0, 0), keys=(0,), **kw):
        self.h = frames[0].shape[0]
        self.w = frames[0].shape[1] if bpp == 32 else frames[0].shape[1] // 3
        self.frames, self.bpp, self.kw = frames, bpp, kw
        self.rowbytes = self.w * bpp // 8
        self.pitch = self.w * 4 if bpp == 32 else (self.rowbytes + 3) & ~3
        enc = O.OracleCodec(self.w, self.h, bpp, **kw)
        enc.set_p_race(*race)
        ref = [enc.compress(f, key=(t in keys)) for t, f in enumerate(frames)]
        self.packets, self.ftypes = [p for p, _ in ref], [ft for _, ft in ref]
        self.rows = np.stack([np.asarray(f).reshape(self.h, -1)[:, :self.rowbytes] for f in frames])
        dec = O.OracleCodec(self.w, self.h, bpp, **kw)
        outs = []
        for p, ft in zip(self.packets, self.ftypes):
            r, out = dec.decompress(p, ft)
            assert r == 1
            outs.append(out.reshape(self.h, self.pitch)[:, :self.rowbytes])
        self.oracle = np.stack(outs)
        assert np.array_equal(self.oracle, self.rows)

    def codec(self):
        return _codec(self.w, self.h, self.bpp, **self.kw)

    def entry(self, codec, a, b):
        import torch
        out = torch.zeros((b - a) * self.pitch * self.h, dtype=torch.uint8, device="cuda")
        return (codec, _dev(self.packets[a:b]), [len(p) for p in self.packets[a:b]], self.ftypes[a:b], self.pitch, out)

    def check(self, out, a, b, what):
        out = out[:(b - a) * self.pitch * self.h]
        got = (out if isinstance(out, np.ndarray) else out.cpu().numpy()).reshape(b - a, self.h, self.pitch)[:, :, :self.rowbytes]
        for t in range(b - a):
            assert np.array_equal(got[t], self.oracle[a + t]) and np.array_equal(got[t], self.rows[a + t]), (what, a + t)


def _desktop(w, h, n, bpp=32, **kw):
    seq = DesktopSequence(w, h, **kw)
    return [seq.frame(t) if bpp == 32 else pack24(seq.frame24(t)) for t in range(n)]


_RACE = None


def race_streams():
    """(name, Stream) for the race cases, built once: W in {2, 6, 16, 32}, scrolling / moving windows, static pictures with
    noise patches, a 2-block-row picture with W > nby, odd widths, 640x480, RGB24, non-default motion ranges, one GOP of
    100 P-frames"""
    global _RACE
    if _RACE is None:
        _RACE = [("desktop_160x120_w2", Stream(_desktop(160, 120, 10, seed=3), race=(2, 1))),
                 ("desktop_99x61_rgb24_w6", Stream(_desktop(99, 61, 10, 24, seed=4), 24, race=(6, 2))),
                 ("desktop_640x480_w16", Stream(_desktop(640, 480, 6, seed=5), race=(16, 3))),
                 ("static_noise_321x200_w32", Stream(_desktop(321, 200, 8, seed=6, static=True, noise_fraction=0.03), race=(32, 4))),
                 ("two_rows_64x20_w6", Stream(foreign.two_row_frames(8), race=(6, 5))),
                 ("ranges_200x150_w16", Stream(_desktop(200, 150, 10, seed=7), race=(16, 6), high_range=(40, 24), low_range=(4, 2))),
                 ("ranges_150x90_rgb24_w32", Stream(_desktop(150, 90, 8, 24, seed=8), 24, race=(32, 7), high_range=(300, 17), low_range=(12, 1))),
                 ("long_gop_160x120_w6", Stream(_desktop(160, 120, 101, seed=9), race=(6, 8)))]
    return _RACE


def test_race_streams_differ_from_canonical():
    """(the cases below are not canonical streams in disguise)"""
    for name, s in race_streams():
        can = Stream(s.frames, s.bpp, **s.kw)
        differ = sum(a != b for a, b in zip(s.packets, can.packets))
        assert differ >= (30 if name.startswith("long_gop") else 2), (name, differ)


def test_race_streams_per_frame_api():
    for name, s in race_streams():
        dec = s.codec()
        for t, (p, ft) in enumerate(zip(s.packets, s.ftypes)):
            r, out = dec.DecompressFrame(p, ft)
            assert r == 1, (name, t)
            got = out.reshape(s.h, s.pitch)[:, :s.rowbytes]
            assert np.array_equal(got, s.oracle[t]) and np.array_equal(got, s.rows[t]), (name, t)


def test_race_streams_batch_over_uneven_calls():
    sizes = [1, 4, 2, 7, 3, 5]  # calls that start mid-GOP
    for name, s in race_streams():
        dec = s.codec()
        a, k = 0, 0
        while a < len(s.packets):
            b = min(len(s.packets), a + sizes[k % len(sizes)])
            _, packets, sz, ft, pitch, _ = s.entry(dec, a, b)
            r, out = dec.DecompressBatch(packets, sz, ft, pitch)
            assert r == b - a, (name, a, r)
            s.check(out, a, b, name)
            a, k = b, k + 1


def test_race_streams_side_by_side_with_canonical_streams():
    """every race stream and two canonical ones in shared launches, over two calls (the second starts mid-GOP)"""
    from screenpressor_amd.codec import decompress_streams
    ss = [s for _, s in race_streams()] + [Stream(_desktop(160, 120, 10, seed=3)), Stream(_desktop(99, 61, 10, 24, seed=4), 24)]
    codecs = [s.codec() for s in ss]
    for call in range(2):
        cuts = [(0, 3) if call == 0 else (3, len(s.packets)) for s in ss]
        res = decompress_streams([s.entry(c, a, b) for s, c, (a, b) in zip(ss, codecs, cuts)])
        for i, (s, (a, b), (r, out)) in enumerate(zip(ss, cuts, res)):
            assert r == b - a, (i, call, r)
            s.check(out, a, b, (i, call))


def _check_entries(gpu, ora):
    ge, oe = gpu.debug_entries(), ora.entries()
    n = min(len(ge), len(oe))
    d = np.nonzero((ge[:n] != oe[:n]).any(axis=1))[0]
    assert len(ge) == len(oe) and len(d) == 0, f"entries differ: gpu {len(ge)} oracle {len(oe)} first at {d[:5]}"


@pytest.mark.parametrize("workers", [5, 6, 7, 12, 16, 24, 32])
def test_key_frames_of_wide_worker_pools(workers):
    """uneven GetSegment bands (squad.cpp:16-31) over heights 2W, 2W + 1, 100, 101 (and 1080 for some W; RGB24 for W = 12):
    the GPU encoder's bytes equal the oracle's, and a decoder that does not know W gets the picture back"""
    cases = [(72, 2 * workers, 32), (72, 2 * workers + 1, 32), (90, 100, 32), (91, 101, 32)]
    if workers in (7, 24):
        cases.append((1920, 1080, 32))
    if workers == 12:
        cases.append((91, 101, 24))
    for w, h, bpp in cases:
        f = _desktop(w, h, 1, bpp, seed=workers + h)[0]
        ora = O.OracleCodec(w, h, bpp, workers=workers)
        want, _ = ora.compress(f, key=True)
        gpu = _codec(w, h, bpp, workers=workers)
        got, ft = gpu.CompressFrame(f, 0)
        if got != want:
            _check_entries(gpu, ora)
        assert ft == 0 and got == want, (w, h, bpp)
        dec = _codec(w, h, bpp)
        r, out = dec.DecompressFrame(got, 0)
        rb = w * bpp // 8
        assert r == 1 and np.array_equal(out.reshape(h, -1)[:, :rb], np.asarray(f).reshape(h, -1)[:, :rb]), (w, h, bpp)


def _exact_streams():
    """(exact key frame of 1 block, of 2 blocks, the (key, P of 1 block, next) GOP) as oracle streams, entry counts asserted"""
    out = []
    for f, k in ((foreign.exact_key_1(), 1), (foreign.exact_key_2(), 2)):
        s = Stream([f])
        ora = O.OracleCodec(s.w, s.h, 32)
        ora.compress(f, key=True)
        assert len(ora.entries()) == k * foreign.BLOCK
        out.append(s)
    frames = foreign.exact_p_pair()
    s = Stream(frames)
    ora = O.OracleCodec(s.w, s.h, 32)
    ora.compress(frames[0], key=True)
    ora.compress(frames[1], key=False)
    assert s.ftypes == [0, 1, 1] and len(ora.entries()) == foreign.BLOCK
    out.append(s)
    return out


def test_frames_of_exactly_k_blocks():
    from screenpressor_amd.codec import decompress_streams
    k1, k2, gop = _exact_streams()
    # the GPU encoder writes the oracle's bytes
    for s, frames in ((k1, [foreign.exact_key_1()]), (k2, [foreign.exact_key_2()]), (gop, foreign.exact_p_pair())):
        enc = s.codec()
        for t, f in enumerate(frames):
            got, ft = enc.CompressFrame(f, 0 if t == 0 else 1)
            assert ft == s.ftypes[t] and got == s.packets[t], (s.w, s.h, t)
    # per frame
    for s in (k1, k2, gop):
        dec = s.codec()
        for t, (p, ft) in enumerate(zip(s.packets, s.ftypes)):
            r, out = dec.DecompressFrame(p, ft)
            assert r == 1
            s.check(out, t, t + 1, ("frame", s.w, s.h))
    # batches: the exact frame last in the packet buffer, then in the middle of it (with the frame after it decoded too)
    for a, b in ((0, 2), (0, 3), (1, 3)):
        dec = gop.codec()
        if a:
            assert dec.DecompressFrame(gop.packets[0], 0)[0] == 1
        _, packets, sz, ft, pitch, _ = gop.entry(dec, a, b)
        r, out = dec.DecompressBatch(packets, sz, ft, pitch)
        assert r == b - a
        gop.check(out, a, b, ("batch", a, b))
    for s in (k1, k2):  # key frames: after a canonical key frame, and before one
        other = Stream(_desktop(s.w, s.h, 1, seed=12))
        for order in ((other, s), (s, other)):
            dec = s.codec()
            packets = [order[0].packets[0], order[1].packets[0]]
            r, out = dec.DecompressBatch(_dev(packets), [len(p) for p in packets], [0, 0], s.pitch)
            assert r == 2
            for i, src in enumerate(order):
                src.check(out[i * s.pitch * s.h:], 0, 1, ("batch", s.h, i))
    # streams: the exact frame last in its stream's call; the frame after it in the next call
    can = Stream(_desktop(160, 120, 4, seed=13))
    ss, codecs = [gop, k1, k2, can], [gop.codec(), k1.codec(), k2.codec(), can.codec()]
    res = decompress_streams([gop.entry(codecs[0], 0, 2), k1.entry(codecs[1], 0, 1), k2.entry(codecs[2], 0, 1), can.entry(codecs[3], 0, 2)])
    for (a, b), s, (r, out) in zip(((0, 2), (0, 1), (0, 1), (0, 2)), ss, res):
        assert r == b - a
        s.check(out, a, b, ("streams", s.w, s.h))
    res = decompress_streams([gop.entry(codecs[0], 2, 3), can.entry(codecs[3], 2, 4)])
    for (a, b), s, (r, out) in zip(((2, 3), (2, 4)), (gop, can), res):
        assert r == b - a
        s.check(out, a, b, ("streams after", s.w, s.h))
