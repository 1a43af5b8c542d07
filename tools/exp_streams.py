#!/usr/bin/env python3
"""Many independent streams decoded in one launch (scpr_decompress_streams) against the same streams decoded one codec after another
(scpr_decompress_batch).

  python tools/exp_streams.py [--S 1,8,64,256] [--frames 60] [--round r6a]

S distinct one-GOP 1080p RGB32 streams (DesktopSequence, seed = stream index + 1, `--frames` frames each, a key frame and P-frames)
are encoded once (the largest S; the smaller S take the first streams), then decoded by S decoder codecs
  (a) serial:  S consecutive DecompressBatch calls,
  (b) streams: one decompress_streams call,
per S.  Reported per S: aggregate decode MPix/s of (a) and (b), per-stream milliseconds per P-frame, and whether every decoded
picture equals its input (a checksum of every input frame, computed where the frame is rendered, against the same checksum of the
decoded picture on the GPU; (a) and (b) are also compared byte for byte).  The line goes to profiles/<round>_streams.json.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from screenpressor_amd.synth import DesktopSequence  # noqa: E402

W, H = 1920, 1080
_MOD = np.uint64(0xFFFFFFFB)  # checksum: sum of word_i * (i % 65521 + 1) over the frame's 32-bit words, mod a 32-bit prime


def _weights(n):
    return (np.arange(n, dtype=np.uint64) % np.uint64(65521)) + np.uint64(1)


def checksum_np(frame: np.ndarray, wts: np.ndarray) -> int:
    w = frame.reshape(-1).view(np.uint32).astype(np.uint64)
    return int(np.sum((w * wts) % _MOD) % _MOD)


def checksum_torch(frames, wts):
    """(k, H*W) int64 words of k pictures -> k checksums (the same arithmetic, on the GPU)"""
    m = 0xFFFFFFFB
    return (((frames * wts[None, :]) % m).sum(dim=1) % m).tolist() if frames.numel() else []


def render(args):
    seed, n = args
    seq = DesktopSequence(W, H, seed=seed)
    wts = _weights(W * H)
    frames = np.stack([seq.frame(t) for t in range(n)])
    return seed, frames, [checksum_np(f, wts) for f in frames]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", default="1,8,64,256")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--round", default="r6a")
    ap.add_argument("--workers", type=int, default=min(32, os.cpu_count() or 1), help="host processes rendering the frames")
    a = ap.parse_args()
    import torch
    from screenpressor_amd.codec import ScreenCodec, decompress_streams
    Ss = [int(x) for x in a.S.split(",")]
    smax, n = max(Ss), a.frames
    ftypes_in = [0] + [1] * (n - 1)
    t0 = time.time()
    encoders = [ScreenCodec(0).Init(W, H, 32) for _ in range(4)]
    streams = [None] * smax  # (packets on the device, sizes, ftypes, input checksums)
    with mp.get_context("spawn").Pool(a.workers) as pool:
        for seed, frames, sums in pool.imap(render, [(s + 1, n) for s in range(smax)]):
            enc = encoders[seed % len(encoders)].Init(W, H, 32)  # (a fresh stream: Init drops what the last one left)
            pk, sizes, fts = enc.CompressBatch(torch.from_numpy(frames).cuda(), ftypes_in)
            streams[seed - 1] = (pk, [int(x) for x in sizes], fts, sums)
    enc_s = time.time() - t0
    pkt_bytes = sum(int(p.numel()) for p, _, _, _ in streams)
    print(f"encoded {smax} streams x {n} frames in {enc_s:.1f} s ({pkt_bytes / 1e6:.1f} MB of packets)", flush=True)
    wts = torch.from_numpy(_weights(W * H).astype(np.int64)).cuda()
    frame_bytes = W * H * 4
    decoders = [ScreenCodec(0).Init(W, H, 32) for _ in range(smax)]
    outs = [torch.empty(n * frame_bytes, dtype=torch.uint8, device="cuda") for _ in range(smax)]
    free, total = torch.cuda.mem_get_info()
    print(f"memory: {smax} outputs of {n * frame_bytes / 2**30:.2f} GiB; device {free / 2**30:.1f} GiB free of {total / 2**30:.1f} GiB", flush=True)

    def verify(i):
        o = outs[i].view(torch.int32).view(n, W * H).to(torch.int64) & 0xFFFFFFFF
        return checksum_torch(o, wts) == streams[i][3]

    results = []
    for S in Ss:
        for i in range(S):  # fresh decoders for each form and S (one stream, one GOP)
            decoders[i].Init(W, H, 32)
        torch.cuda.synchronize()
        t = time.time()
        for i in range(S):
            pk, sizes, fts, _ = streams[i]
            r, _ = decoders[i].DecompressBatch(pk, sizes, fts, out=outs[i], sync=False)
            assert r == n, (i, r)
        torch.cuda.synchronize()
        ta = time.time() - t
        exact_a = all(verify(i) for i in range(S))
        keep = [outs[i].clone() for i in range(min(S, 8))]  # (a) against (b), byte for byte, on the first streams
        for i in range(S):
            decoders[i].Init(W, H, 32)
            outs[i].zero_()
        torch.cuda.synchronize()
        t = time.time()
        res = decompress_streams([(decoders[i], streams[i][0], streams[i][1], streams[i][2], None, outs[i]) for i in range(S)], sync=False)
        torch.cuda.synchronize()
        tb = time.time() - t
        assert all(r == n for r, _ in res), [r for r, _ in res if r != n][:4]
        exact_b = all(verify(i) for i in range(S)) and all(torch.equal(keep[i], outs[i]) for i in range(len(keep)))
        tm, st = decoders[0].last_timing()
        px = S * n * W * H
        row = {"S": S, "frames_per_stream": n, "serial_s": round(ta, 4), "streams_s": round(tb, 4),
               "serial_mpix_s": round(px / ta / 1e6, 1), "streams_mpix_s": round(px / tb / 1e6, 1),
               "serial_ms_per_pframe_per_stream": round(ta / S / n * 1e3, 3), "streams_ms_per_pframe_per_stream": round(tb / n * 1e3, 3),
               "streams_decode_kernel_ms": round(st.get("decode", 0.0), 2), "streams_unpack_ms": round(st.get("unpack", 0.0), 2),
               "exact_serial": bool(exact_a), "exact_streams": bool(exact_b)}
        print(json.dumps(row), flush=True)
        results.append(row)
        del keep
    base = next((r for r in results if r["S"] == 1), None)
    line = {"tool": "tools/exp_streams.py", "width": W, "height": H, "bpp": 32, "frames_per_stream": n, "gop": "one per stream",
            "encode_s": round(enc_s, 1), "rows": results,
            "streams_speedup_over_one_stream": {str(r["S"]): round(r["streams_mpix_s"] / base["streams_mpix_s"], 2) for r in results} if base else None}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"{a.round}_streams.json")
    with open(path, "w") as f:
        json.dump(line, f, indent=1)
    print(json.dumps(line))
    print("wrote", path)


if __name__ == "__main__":
    main()
