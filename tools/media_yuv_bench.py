"""Send/receive leg of the media plane, packed RGB against I420
(profiles/media_yuv.md).

  send leg:    engine output tensor on the device -> H264SwCodec.encode returns
  receive leg: H264SwCodec.decode of an access unit -> frame resident on the
               device as RGB (upload, plus ops.i420_to_rgb_u8 in I420 mode),
               device synchronised

Wall clock per frame with a device synchronise at both ends, one process,
median and p10/p90 over --frames frames after --warmup. The engine itself is
not in the loop: the frames are a fixed set of synthetic pictures, the same
in both modes (the I420 set is the conversion of the RGB set).

    python tools/media_yuv_bench.py --size 512 --frames 300
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ai_rtc_agent_amd import ops  # noqa: E402
from ai_rtc_agent_amd.media.codec import H264SwCodec  # noqa: E402


def pictures(n, size, device):
    """Smooth moving gradients plus a little noise: codes like video, not
    like white noise."""
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    out = []
    for k in range(n):
        base = torch.stack([(xx + 3 * k) % 256, (yy + 2 * k) % 256,
                            ((xx + yy) // 2 + k) % 256], dim=-1).float()
        base += torch.randn((size, size, 3), generator=g) * 4
        out.append(base.clamp(0, 255).to(torch.uint8).to(device))
    return out


def stats(ms):
    ms = sorted(ms)
    return (statistics.median(ms), ms[len(ms) // 10], ms[len(ms) * 9 // 10])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=512)
    p.add_argument("--frames", type=int, default=300)
    p.add_argument("--warmup", type=int, default=30)
    a = p.parse_args()
    dev = "cuda"
    rgb = pictures(16, a.size, dev)
    yuv = [ops.rgb_u8_to_i420(f) for f in rgb]
    total = a.frames + a.warmup
    rows = []
    for mode, frames in (("rgb", rgb), ("i420", yuv)):
        codec = H264SwCodec(yuv=(mode == "i420"))
        send, aus = [], []
        for k in range(total):
            f = frames[k % len(frames)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            au = codec.encode(f)
            send.append((time.perf_counter() - t0) * 1e3)
            aus.append(au)
        recv = []
        for au in aus:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t = codec.decode(au).to(dev, non_blocking=True)
            if mode == "i420":
                t = ops.i420_to_rgb_u8(t)
            torch.cuda.synchronize()
            recv.append((time.perf_counter() - t0) * 1e3)
        assert t.shape == (a.size, a.size, 3)
        rows.append((mode, stats(send[a.warmup:]), stats(recv[a.warmup:]),
                     sum(map(len, aus)) // len(aus)))
    print(f"| mode | send median (p10-p90) ms | receive median (p10-p90) ms | mean AU bytes |")
    print("|---|---|---|---|")
    for mode, s, r, nb in rows:
        print(f"| {mode} | {s[0]:.3f} ({s[1]:.3f}-{s[2]:.3f}) | "
              f"{r[0]:.3f} ({r[1]:.3f}-{r[2]:.3f}) | {nb} |")


if __name__ == "__main__":
    main()
