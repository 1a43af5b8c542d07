"""CPU tests of the ORACLE (oracle/): the rANS arithmetic pinned against the
reference's own rans_byte.h (its answers stored in golden/ref_rans.json, and
oracle/_ref itself where it was built from the reference tree), the two known answers SURVEY.md §8c records from the real
reference, and lossless round trips over the edge cases the format has."""
import ctypes as C
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

import foreign_streams as foreign
import oracle_api as O
from screenpressor_amd.synth import DesktopSequence, pack24

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ref_rans", os.path.join(GOLD, "make_ref_rans.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
REF_RANS = json.load(open(os.path.join(GOLD, "ref_rans.json")))  # the reference's answers to the cases below (make_ref_rans.py)
REF_SO = os.path.join(O.ORACLE_DIR, "_ref", "librefrans.so")


def _rans_decode_values(data, e):
    """the byte-wise rANS decoder (32-bit state, lower bound 2^23, 12-bit probabilities) over `data`: (bytes used, the 12-bit
    value or raw byte taken per entry)"""
    buf = data + b"\0" * 8
    x, p = int.from_bytes(buf[:4], "little"), 4
    vals = np.zeros(len(e), dtype=np.uint16)
    for i, (freq, cum) in enumerate(e.tolist()):
        if freq:
            vals[i] = x & 4095
            x = freq * (x >> 12) + (x & 4095) - cum
            while x < 1 << 23:
                x, p = (x << 8) | buf[p], p + 1
        else:
            vals[i], p = buf[p], p + 1
    return p, vals


@pytest.mark.parametrize("n", R.BLOCK_NS)
def test_rans_block_matches_reference_header(n):
    """oracle rANS restatement == reference rans_byte.h driven as ransmt.h:116-134 does (its bytes as stored in
    golden/ref_rans.json, and live where oracle/_ref is built)"""
    want = REF_RANS["blocks"][str(n)]
    e = R.block_entries(n)
    mine = O.rans_block(e)
    assert (len(mine), R.sha256(mine)) == (want["bytes"], want["sha256"])
    # and the decoder walks those bytes back through every interval, taking what the reference decoder took
    used, vals = _rans_decode_values(mine, e)
    assert (used, R.sha256(vals.astype("<u2").tobytes())) == (want["used"], want["values_sha256"])
    assert used == len(mine)
    coded = e[:, 0] > 0
    assert np.all(vals[coded] >= e[coded, 1]) and np.all(vals[coded] < e[coded, 1].astype(int) + e[coded, 0])
    assert np.array_equal(vals[~coded], e[~coded, 1])
    if os.path.exists(REF_SO):
        ref = R.Ref(REF_SO)
        assert ref.block(e) == mine
        rused, rvals = ref.decode_values(mine, e)
        assert rused == used and np.array_equal(rvals, vals)


def test_product_rans_algebra_is_the_reference_headers_symbol_form():
    """rans_byte.h:171-241, :255-278 (RansEncSymbolInit / RansEncPutSymbol) against the table and the step the
    product's rANS kernels implement (csrc/scpr_model.hpp rans_rcp; k_rans / k_rans_s): for EVERY freq 1..4096 the reciprocal,
    the shift, bias - start, x_max and 4096 - freq are the header's, and one step from a spread of states and starts gives the
    header's new state and bytes - the header's answers as stored in golden/ref_rans.json, and live where oracle/_ref is built.
    (The kernels themselves are compared with the oracle on the GPU; this moves their arithmetic from "equals the oracle, which
    equals the header's other form" to "equals the header".)"""
    from screenpressor_amd import build as B
    hm = C.CDLL(B.build_host_harness())
    hm.hm_rans_step.restype = C.c_uint32
    h3, hb, hn = (C.c_uint32 * 3)(), (C.c_uint8 * 8)(), C.c_int()

    def params(freq, start):
        hm.hm_rans_params(freq, h3)
        return (freq << 19) & 0xFFFFFFFF, h3[0], h3[1], h3[2], 4096 - freq

    def step(x, start, freq):
        s = hm.hm_rans_step(x, start, freq, hb, C.byref(hn))
        return (s, hn.value) + tuple(hb[:hn.value])
    mine = list(R.algebra_records(params, step))
    if os.path.exists(REF_SO):
        ref = R.Ref(REF_SO)
        for (freq, start, x), r in mine:
            assert (ref.params(freq, start) if x is None else ref.step(x, start, freq)) == r, (freq, start, x)
    assert (len(mine), R.digest(mine)) == (REF_RANS["algebra"]["records"], REF_RANS["algebra"]["sha256"])


def test_survey_known_answers():
    """SURVEY.md §8c, observed on the compiled reference: an I-frame starts with
    three raw bytes of pixel 0 then N[0](1) = (16,16); a P-frame with one
    changed pixel at (3,5) is block 0 type 2, rect 3,5-4,6, exactly 15 entries."""
    enc = O.OracleCodec(64, 48, 32)
    rng = np.random.default_rng(5)
    f = np.full((48, 64, 4), 255, np.uint8)
    f[..., :3] = rng.integers(0, 256, (48, 64, 3))
    f[0, 0, :3] = (0, 0, 200)
    data, ft = enc.compress(f, key=True)
    assert ft == 0 and data[0] == 0x32
    e = enc.entries()
    assert e[:4].tolist() == [[0, 0], [0, 0], [0, 200], [16, 16]]
    g = f.copy()
    g[5, 3, :3] = (9, 9, 9)
    data, ft = enc.compress(g, key=False)
    assert ft == 1 and data[0] == 0x01
    bt, rect, mv = enc.blocks()
    assert bt[0] == 2 and rect[:, 0].tolist() == [3, 5, 4, 6]
    assert len(enc.entries()) == 15


def _roundtrip(frames, w, h, bpp=32, keys=(0,), loss=0, workers=1, pitch=None):
    enc = O.OracleCodec(w, h, bpp, loss=loss, workers=workers)
    dec = O.OracleCodec(w, h, bpp, loss=loss, workers=workers)
    sizes, types = [], []
    hsh = hashlib.sha256()
    for t, f in enumerate(frames):
        data, ft = enc.compress(f, key=(t in keys))
        r, out = dec.decompress(data, ft)
        assert r == 1
        sizes.append(len(data))
        types.append(ft)
        hsh.update(data)
        yield t, f, out, data, ft
    _roundtrip.last = (sizes, types, hsh.hexdigest())


@pytest.mark.parametrize("w,h", [(64, 48), (100, 37), (33, 17), (640, 480), (3, 2), (17, 16)])
def test_roundtrip_desktop_rgb32(w, h):
    seq = DesktopSequence(w, h, seed=3)
    n = 60 if (w, h) == (640, 480) else 8
    for t, f, out, data, ft in _roundtrip([seq.frame(t) for t in range(n)], w, h):
        assert np.array_equal(out.reshape(h, w, 4), f), t
        assert ft == (0 if t == 0 else 1)
        assert data[0] in ((0x32, 0x31) if t == 0 else (0x00, 0x01))


def test_rgb24_equals_rgb32_stream_and_padding():
    w, h = 100, 37  # width not a multiple of 4: padded rows
    seq = DesktopSequence(w, h, seed=4)
    f32 = [seq.frame(t) for t in range(6)]
    f24 = [pack24(seq.frame24(t)) for t in range(6)]
    d32 = [d for _, _, _, d, _ in _roundtrip(f32, w, h, 32)]
    outs = list(_roundtrip(f24, w, h, 24))
    assert [d for _, _, _, d, _ in outs] == d32
    for t, f, out, _, _ in outs:
        assert np.array_equal(out.reshape(f.shape), f)  # padding decodes to zero too


def test_flat_frames_and_unchanged_frames():
    w, h = 64, 48
    a = np.full((h, w, 4), 255, np.uint8)
    a[..., :3] = (10, 20, 30)
    b = a.copy()
    b[..., :3] = (11, 20, 30)
    c = a.copy()
    c[7, 9, :3] = (1, 2, 3)
    frames = [a, a, b, c, c, a, c, c]
    packets = []
    for t, f, out, data, ft in _roundtrip(frames, w, h, keys=()):
        assert np.array_equal(out.reshape(h, w, 4), f), t
        packets.append((data, ft))
    assert packets[0] == (bytes([0x31, 10, 20, 30]), 0)   # flat key frame even though P was requested
    assert packets[1] == (bytes([0x31, 10, 20, 30]), 0)   # repeated flat colour
    assert packets[2] == (bytes([0x31, 11, 20, 30]), 0)
    assert packets[3][1] == 0 and packets[3][0][0] == 0x32  # flat frames do not count: first coded frame is I
    assert packets[4] == (b"\x00", 1)                       # unchanged P-frame
    assert packets[5][0] == bytes([0x31, 10, 20, 30])
    assert packets[6][1] == 1 and packets[6][0][0] == 0x01  # P after a flat frame
    assert packets[7] == (b"\x00", 1)


def test_motion_search_scroll():
    w, h = 320, 240
    rng = np.random.default_rng(7)
    tex = rng.integers(0, 256, (h + 64, w, 3), dtype=np.uint8)
    frames = []
    for t in range(5):
        f = np.full((h, w, 4), 255, np.uint8)
        f[..., :3] = tex[3 * t:3 * t + h]
        frames.append(f)
    enc = O.OracleCodec(w, h, 32)
    dec = O.OracleCodec(w, h, 32)
    for t, f in enumerate(frames):
        data, ft = enc.compress(f, key=(t == 0))
        r, out = dec.decompress(data, ft)
        assert r == 1 and np.array_equal(out.reshape(h, w, 4), f)
        if t:
            bt, rect, mv = enc.blocks()
            inner = bt.reshape(15, 20)[:-1]  # bottom rows have no source in prev
            assert np.all(inner >= 3)
            assert set(zip(mv[0][bt >= 3].tolist(), mv[1][bt >= 3].tolist())) == {(0, 3)}
            assert len(data) < 20 * 16 * 16 * 3 + 2000  # only the bottom block row is coded as pixels


def test_multi_block_rans():
    """a frame with more than 131072 coder entries: several rANS blocks (ransmt.h:38)"""
    w, h = 320, 240
    seq = DesktopSequence(w, h, seed=5, noise_fraction=0.6)
    enc = O.OracleCodec(w, h, 32)
    dec = O.OracleCodec(w, h, 32)
    for t in range(3):
        f = seq.frame(t)
        data, ft = enc.compress(f, key=(t == 0))
        assert len(enc.entries()) > 131072
        r, out = dec.decompress(data, ft)
        assert r == 1 and np.array_equal(out.reshape(h, w, 4), f)


@pytest.mark.parametrize("loss", [1, 3])
def test_lossy_roundtrip(loss):
    w, h = 100, 37
    seq = DesktopSequence(w, h, seed=6)
    mask = (~((1 << loss) - 1)) & 0xFF
    corr = (1 << loss) >> 1
    for t, f, out, data, ft in _roundtrip([seq.frame(t) for t in range(4)], w, h, loss=loss):
        want = f.copy()
        want[..., :3] = (f[..., :3] & mask) | corr
        assert np.array_equal(out.reshape(h, w, 4), want)


def test_rgb16_roundtrip():
    w, h = 64, 48
    rng = np.random.default_rng(8)
    px = rng.integers(0, 1 << 15, (h, w), dtype=np.uint16)
    px[:, : w // 2] = 0x1234
    enc = O.OracleCodec(w, h, 16)
    dec = O.OracleCodec(w, h, 16)
    data, ft = enc.compress(px.view(np.uint8), key=True)
    r, out = dec.decompress(data, ft)
    assert r == 1 and np.array_equal(out.view(np.uint16).reshape(h, w), px)


def test_worker_count_is_bitstream_visible_for_key_frames():
    """screencap.cpp:365-388: runs are cut at band starts, one band per worker"""
    w, h = 128, 96
    f = DesktopSequence(w, h, seed=9).frame(0)
    streams = {}
    for nw in (1, 2, 4, 8):
        enc = O.OracleCodec(w, h, 32, workers=nw)
        dec = O.OracleCodec(w, h, 32, workers=1)
        data, ft = enc.compress(f, key=True)
        r, out = dec.decompress(data, ft)
        assert r == 1 and np.array_equal(out.reshape(h, w, 4), f)
        streams[nw] = data
    assert len(set(streams.values())) > 1


def test_decoder_refusals():
    w, h = 64, 48
    dec = O.OracleCodec(w, h, 32)
    r, _ = dec.decompress(b"\x01abc", 1)
    assert r == 0  # P-frame before any key frame (screencap.cpp:1699)
    r, _ = dec.decompress(bytes([0x02, 0, 0, 0, 0]), 0)
    assert r < 0   # version 1 stream: BadVersionException (screencap.cpp:1589-1590)


def _model_sequences():
    rng = np.random.default_rng(11)
    yield rng.integers(0, 256, 5000)                          # dense: kinds 1,2,3 -> 7
    yield rng.choice([3, 200], 3000)                          # kind 4
    yield rng.choice(rng.integers(0, 256, 10), 4000)          # kind 5
    yield rng.choice(rng.integers(0, 256, 30), 6000)          # kind 6
    yield np.concatenate([rng.choice([5, 6, 7], 500), rng.choice(np.arange(0, 256, 7), 4000)])  # 4 -> 5 -> 6 -> 7
    yield np.concatenate([np.arange(40), np.arange(40), rng.integers(0, 64, 3000)])            # kind 2 -> 6 (S=64)
    yield np.concatenate([np.arange(20), [1, 1, 0, 255], rng.integers(0, 32, 2000)])           # kind 2 -> 6 (S=32), symbol 1
    yield np.concatenate([np.arange(100), np.arange(100), rng.integers(0, 256, 2000)])         # kind 3 -> 7
    yield np.concatenate([rng.choice([9, 1], 9000), rng.integers(0, 256, 300), rng.choice([9, 1], 3000)])  # heavy rescaling
    z = rng.zipf(1.3, 20000)
    yield np.minimum(z, 255)                                  # skewed


@pytest.mark.parametrize("f0", [32, 64])
def test_model_encoder_decoder_agree(f0):
    """the decoder-side model walk (sorted tables, bucket search) reproduces the
    encoder-side intervals (hash tables) symbol for symbol: ans_contexts.cpp:34-74"""
    for k, seq in enumerate(_model_sequences()):
        syms = np.asarray(seq, dtype=np.uint8)
        if f0 == 64 and k == 5:
            continue  # v3 with > 60 unique symbols overflows the 12-bit scale (reference asserts, ans_contexts.h:501)
        ivl = O.chain_colour(syms, f0)
        coded = ivl[:, 0] > 0
        assert np.all(ivl[coded, 0].astype(int) + ivl[coded, 1] <= 4096), k
        assert O.chain_colour_dec(ivl, syms, f0, probe=0) == 0, k
        assert O.chain_colour_dec(ivl, syms, f0, probe=1) == 0, k


def test_fixed_model_known_answers():
    """ans_contexts.h:1114-1131 renew values; SURVEY Appendix B"""
    for nsym, fr in [(5, 819), (6, 682), (16, 256), (256, 16), (512, 8)]:
        out = O.chain_fixed(nsym, [0, nsym - 1, 1])
        assert out[0].tolist() == [fr, 0]
        assert out[1].tolist() == [fr, fr * (nsym - 1)]
        assert out[2].tolist() == [fr, fr]
    # after enough hits the counts become the frequencies: symbol 0 dominates
    out = O.chain_fixed(256, np.zeros(400, np.uint16))
    assert out[0, 0] == 16 and out[-1, 0] > 3000 and np.all(out[:, 1] == 0)


def test_version2_range_coder_round_trip():
    """UseRC + RangeCoderSub restated (decode side is what the product implements; the encoder exists to make
    streams): lossless round trip over key, P, unchanged and flat frames, header bytes of version 2."""
    w, h = 100, 37
    seq = DesktopSequence(w, h, seed=8, sparkles=20)
    enc, dec = O.OracleCodec(w, h, 32, version=2), O.OracleCodec(w, h, 32)
    flat = np.full((h, w, 4), 255, np.uint8)
    frames = [seq.frame(0), seq.frame(1), seq.frame(1), flat, seq.frame(2), seq.frame(3)]
    heads = []
    for t, f in enumerate(frames):
        p, ft = enc.compress(f, key=(t == 0))
        heads.append(p[0])
        r, out = dec.decompress(p, ft)
        assert r == 1 and np.array_equal(out.reshape(h, w, 4)[..., :3], f[..., :3]), t
    assert heads == [0x12, 0x01, 0x00, 0x11, 0x01, 0x01]


def test_threaded_two_stage_shape_keeps_the_bytes():
    """The CPU baseline's multi-thread form (row bands of a key frame on a pool, squad.cpp:116-130, and one coder thread
    taking the full 131072-entry blocks, ransmt.h:92-105) must give the bytes of the one-thread form at the same
    `workers`: key frames with several coder blocks, and P-frames behind them."""
    from screenpressor_amd.synth import DesktopSequence
    w, h, n = 640, 480, 4
    fr = DesktopSequence(w, h, seed=5, noise_fraction=0.6).frames(n).reshape(n, -1)
    for workers in (1, 4):
        a = O.time_stream(fr, w, h, 32, 2, workers=workers, threads=1)
        b = O.time_stream(fr, w, h, 32, 2, workers=workers, threads=4)
        assert a["bad"] == 0 and b["bad"] == 0
        assert a["fnv"] == b["fnv"] and list(a["sizes"]) == list(b["sizes"]) and a["sizes"].max() > 2 * 131072 // 4
    enc = O.OracleCodec(w, h, 32, workers=4)
    enc.set_threads(4)
    one = O.OracleCodec(w, h, 32, workers=4)
    f = DesktopSequence(w, h, seed=5, noise_fraction=0.6).frame(0)
    assert enc.compress(f, key=True) == one.compress(f, key=True)
    hv = 1469598103934665603  # (the checksum helper bench.py's parity field uses: same recurrence as spo_time_stream's)
    for b in b"abc":
        hv = ((hv ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert O.fnv1a(b"abc") == hv


# ---- streams the canonical encoder never writes (tests/foreign_streams.py) ----
def _race_stream(frames, workers, seed, **kw):
    h, w = frames[0].shape[:2]
    enc = O.OracleCodec(w, h, 32, **kw)
    enc.set_p_race(workers, seed)
    return [enc.compress(f, key=(t == 0)) for t, f in enumerate(frames)]


def _decodes_losslessly(packets, frames, **kw):
    h, w = frames[0].shape[:2]
    dec = O.OracleCodec(w, h, 32, **kw)
    for (p, ft), f in zip(packets, frames):
        r, out = dec.decompress(p, ft)
        if r != 1 or not np.array_equal(out.reshape(h, w, 4), f):
            return False
    return True


def _scroll_frames(n, w=160, h=96):
    tex = np.random.default_rng(7).integers(0, 256, (h + 3 * n, w, 3), dtype=np.uint8)
    out = []
    for t in range(n):
        f = np.full((h, w, 4), 255, np.uint8)
        f[..., :3] = tex[3 * t:3 * t + h]
        out.append(f)
    return out


def test_p_race_with_one_worker_is_the_canonical_stream():
    """one worker claims every row in order with every row above Done: the canonical stream, whatever the seed"""
    flat = np.full((96, 160, 4), 255, np.uint8)
    flat[..., :3] = (9, 99, 199)
    cases = [DesktopSequence(160, 120, seed=3).frames(6), DesktopSequence(100, 37, seed=4, noise_fraction=0.1).frames(5),
             _scroll_frames(5), _scroll_frames(2) + [flat, flat] + _scroll_frames(3)]
    for frames in cases:
        can = _race_stream(frames, 0, 0)
        for seed in (1, 2, 0xDEADBEEF):
            assert _race_stream(frames, 1, seed) == can


@pytest.mark.parametrize("workers", [2, 6, 16, 32])
def test_p_race_changes_p_frames_and_every_stream_is_lossless(workers):
    """W workers (the reference's pool on a W-core machine) choose other vectors or none: at least half of the P-frames of a
    moving 320x240 desktop differ from the canonical stream over three timings, and each stream still decodes to its input"""
    frames = DesktopSequence(320, 240, seed=3).frames(8)
    can = _race_stream(frames, 0, 0)
    differ = 0
    for seed in (1, 2, 3):
        got = _race_stream(frames, workers, seed)
        assert got[0] == can[0]  # the key frame is not raced
        differ += sum(a != b for a, b in zip(got[1:], can[1:]))
        assert _decodes_losslessly(got, frames)
    assert differ >= 3 * 7 // 2, differ


def test_p_race_with_more_workers_than_block_rows():
    """64x20 (2 block rows), W = 6: four workers get no band (squad.cpp:24-30) and only steal; row 1's vector depends on
    whether row 0 was Done when it was claimed"""
    frames = foreign.two_row_frames(6)
    can = _race_stream(frames, 0, 0)
    differ = 0
    for seed in range(1, 5):
        got = _race_stream(frames, 6, seed)
        differ += sum(a != b for a, b in zip(got[1:], can[1:]))
        assert _decodes_losslessly(got, frames)
    assert differ >= 4 * 5 // 2, differ


def _decode_exact_and_with_garbage(dec_factory, packets, frames):
    """decode from a heap buffer of exactly each packet's length (a sanitizer build sees any read past it), then with
    different garbage after the packet: the same pictures, and they are the input"""
    outs = []
    for tail in (b"", b"\xff" * 8, bytes(range(37, 45)), b"\0" * 3):
        dec = dec_factory()
        got = []
        for (p, ft), f in zip(packets, frames):
            r, out = dec.decompress(p, ft, tail=tail)
            assert r == 1 and np.array_equal(out.reshape(f.shape), f)
            got.append(out)
        outs.append(got)
    for got in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got, outs[0]))


@pytest.mark.parametrize("k", [1, 2])
def test_key_frame_of_exactly_k_blocks(k):
    """a key frame of exactly k * 131072 entries: no tail block, and the decoder's reload after the last block finds no bytes"""
    f = foreign.exact_key_1() if k == 1 else foreign.exact_key_2()
    h, w = f.shape[:2]
    enc = O.OracleCodec(w, h, 32)
    p, ft = enc.compress(f, key=True)
    assert ft == 0 and len(enc.entries()) == k * foreign.BLOCK
    _decode_exact_and_with_garbage(lambda: O.OracleCodec(w, h, 32), [(p, ft)], [f])


def test_p_frame_of_exactly_one_block_and_the_frame_after_it():
    frames = foreign.exact_p_pair()
    h, w = frames[0].shape[:2]
    enc = O.OracleCodec(w, h, 32)
    packets = []
    for t, f in enumerate(frames):
        packets.append(enc.compress(f, key=(t == 0)))
        if t == 1:
            assert packets[1][1] == 1 and len(enc.entries()) == foreign.BLOCK
    _decode_exact_and_with_garbage(lambda: O.OracleCodec(w, h, 32), packets, frames)
