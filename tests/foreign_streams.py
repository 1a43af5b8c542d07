"""Inputs shared by tests/test_oracle.py and tests/test_gpu_foreign_streams.py: pictures whose streams the canonical encoder
never writes, or writes only at an edge of the format.

- P-frames from a multi-worker reference: OracleCodec.set_p_race(W, seed) replays DecideBlockTypes (screencap.cpp:928-1087)
  for W workers under one seeded thread timing.  `two_row_frames` is a 64x20 picture (2 block rows) whose vector choice
  depends on that timing, for W > nby (GetSegment's `total < N` arm, squad.cpp:24-30).
- Frames of exactly k * 131072 coder entries, which end without a tail block (ransmt.h:83-90): the decoder then loads a
  state from the 4 bytes after the packet (screencap.h:327-331).  Each generator is a flat picture whose first `n` pixels in
  raster order are seeded noise, with `d` pixels set back to a cheaper value to land the count exactly; the tests assert
  the count, so a drift of the encoder or of numpy's generator is caught."""
import numpy as np

FLAT = (40, 80, 120)
BLOCK = 131072


def noisy_flat(w, h, n, seed, d=0):
    """RGB32 picture: FLAT with the first n pixels (raster order) noise from default_rng(seed); pixels 4k+2 (k < d) repeat
    their left neighbour"""
    f = np.empty((h * w, 4), np.uint8)
    f[:] = FLAT + (255,)
    f[:n, :3] = np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)
    for k in range(d):
        f[4 * k + 2, :3] = f[4 * k + 1, :3]
    return f.reshape(h, w, 4)


def exact_key_1():
    """256x200 key frame of exactly 131072 entries"""
    return noisy_flat(256, 200, 26226, 1)


def exact_key_2():
    """256x400 key frame of exactly 2 * 131072 entries"""
    return noisy_flat(256, 400, 52404, 1, d=4)


def exact_p_pair():
    """(key, P, next): 256x200; the P-frame over `key` has exactly 131072 entries, `next` is a small change after it"""
    w, h = 256, 200
    key = np.empty((h * w, 4), np.uint8)
    key[:] = FLAT + (255,)
    key[-1, :3] = (1, 2, 3)  # (not a flat frame)
    p = key.copy()
    p[:26202, :3] = np.random.default_rng(2).integers(0, 256, (26202, 3), dtype=np.uint8)
    for k in range(4):
        p[2 * w + 8 * k + 3, :3] = FLAT  # four pixels keep the previous picture's colour
    key, p = key.reshape(h, w, 4), p.reshape(h, w, 4)
    nxt = p.copy()
    nxt[150:170, 40:90, :3] = (200, 10, 10)
    return key, p, nxt


def two_row_frames(n, w=64, h=20):
    """n RGB32 frames with 2 block rows: row 0 is noise that moves right by 6 pixels a frame, row 1 vertical stripes of
    period 5 that move right by 1.  Canonically row 1 first tries row 0's vector (6 = 1 + 5 fits the stripes); a worker
    that claims row 1 with its own chain and no finished row above finds the nearer vector 1 instead."""
    rng = np.random.default_rng(11)
    tex = rng.integers(0, 256, (16, w + 6 * n, 3), dtype=np.uint8)
    stripes = rng.integers(0, 256, (5, 3), dtype=np.uint8)
    out = []
    for t in range(n):
        f = np.full((h, w, 4), 255, np.uint8)
        f[:16, :, :3] = tex[:, 6 * (n - t):6 * (n - t) + w]
        f[16:, :, :3] = stripes[(np.arange(w) - t) % 5][None]
        out.append(f)
    return out
