"""What the full AutoencoderKL VAE (use_tiny_vae=False) costs.

    python tools/vae_bench.py [--steps vae attention e2e] [--batch 1 8]
                              [--iters 50] [--rounds 3] [--limit 120]
                              [--out FILE]

Random weights at the SD1.5 / SD-Turbo architecture, 512x512, f16.

vae        encode and decode ms per call at each --batch (device events
           around --iters eager calls after warm-up, best of --rounds), next
           to TinyVAE on the same box.
attention  the d=512 one-head attention call at L=4096 (the decoder's and
           encoder's mid block at 512x512), per --batch: the wide-head HIP
           kernel, the unfused route it replaces (two library GEMMs and a
           softmax: torch.baddbmm / softmax / bmm in f16) and torch SDPA, on
           the same random q, k, v, in interleaved rounds in one process.
e2e        frames per second of the headline SD-Turbo config with the tiny
           and with the full VAE, alternating rounds (host clock around work
           that ends in a device synchronise).

Every step has --limit seconds: it stops measuring when that runs out and
reports what it has (marked "truncated"). Needs a GPU: there is no CPU
fallback, a timing from one would say nothing. Prints one JSON line (and
writes it to --out).
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ai_rtc_agent_amd import ops  # noqa: E402
from ai_rtc_agent_amd.config import sd_turbo_config  # noqa: E402
from ai_rtc_agent_amd.engine import StreamDiffusionEngine  # noqa: E402
from ai_rtc_agent_amd.models.taesd import TinyVAE  # noqa: E402
from ai_rtc_agent_amd.models.vae_kl import AutoencoderKLVAE  # noqa: E402


class Deadline:
    def __init__(self, seconds):
        self.end = time.perf_counter() + seconds
        self.hit = False

    def over(self):
        self.hit = self.hit or time.perf_counter() > self.end
        return self.hit


def event_ms(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def step_vae(args, dl):
    out = {"cases": []}
    vaes = {"tiny": TinyVAE().to("cuda", torch.float16).eval(),
            "full": AutoencoderKLVAE().to("cuda", torch.float16).eval()}
    for b in args.batch:
        img = torch.rand(b, 512, 512, 3, device="cuda").half() * 2 - 1
        lat = (torch.randn(b, 64, 64, 4, device="cuda") * 0.18215).half()
        case = {"batch": b}
        with torch.no_grad():
            for name, vae in vaes.items():
                enc, dec = [], []
                for _ in range(args.rounds):
                    if dl.over():
                        break
                    enc.append(event_ms(lambda: vae.encode(img), args.iters))
                    dec.append(event_ms(lambda: vae.decode(lat), args.iters))
                case[f"{name}_encode_ms"], case[f"{name}_decode_ms"] = enc, dec
        out["cases"].append(case)
    out["truncated"] = dl.hit
    return out


def step_attention(args, dl):
    out = {"L": 4096, "d": 512, "cases": []}
    scale = 1.0 / math.sqrt(512)
    for b in args.batch:
        g = torch.Generator().manual_seed(b)
        qkv = torch.randn(b, 4096, 1536, generator=g).half().cuda()
        q, k, v = qkv.chunk(3, dim=-1)   # the model's layout: row stride 1536

        def unfused():
            s = torch.bmm(q, k.transpose(1, 2))
            return torch.bmm(torch.softmax(s.float() * scale, dim=-1).half(), v)

        def unfused_f16():
            return torch.bmm(torch.softmax(torch.bmm(q, k.transpose(1, 2)) * scale,
                                           dim=-1), v)

        def sdpa():
            return F.scaled_dot_product_attention(
                q[:, None], k[:, None], v[:, None], scale=scale)

        arms = {"hip_wide": lambda: ops.attention(q, k, v, 1),
                "unfused_f32_softmax": unfused, "unfused_f16_softmax": unfused_f16,
                "torch_sdpa": sdpa}
        ref = unfused().float()
        case = {"batch": b, "us": {n: [] for n in arms},
                "max_abs_vs_unfused": {
                    n: (f().float().reshape(ref.shape) - ref).abs().max().item()
                    for n, f in arms.items()}}
        for _ in range(args.rounds):
            for n, f in arms.items():
                if dl.over():
                    break
                case["us"][n].append(event_ms(f, args.iters) * 1e3)
        case["median_us"] = {n: sorted(t)[len(t) // 2] for n, t in case["us"].items() if t}
        out["cases"].append(case)
    out["truncated"] = dl.hit
    return out


def step_e2e(args, dl):
    def timed(eng, frame, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            eng(frame)
        eng.sync_output()
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    frame = torch.randint(0, 256, (512, 512, 3), dtype=torch.uint8,
                          generator=torch.Generator().manual_seed(1)).cuda()
    engines = {}
    for name, tiny in (("tiny_vae", True), ("full_vae", False)):
        eng = StreamDiffusionEngine(sd_turbo_config(
            device="cuda", width=512, height=512, use_tiny_vae=tiny))
        eng.prepare()
        timed(eng, frame, 30)   # capture + warm-up
        engines[name] = eng
    fps = {n: [] for n in engines}
    for _ in range(args.rounds):
        for n, eng in engines.items():
            if dl.over():
                break
            fps[n].append(timed(eng, frame, args.iters * 4))
    return {"fps": fps, "best_fps": {n: max(v) for n, v in fps.items() if v},
            "truncated": dl.hit}


STEPS = {"vae": step_vae, "attention": step_attention, "e2e": step_e2e}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", nargs="+", default=list(STEPS), choices=list(STEPS))
    p.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--limit", type=float, default=120.0, help="seconds per step")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_bench needs a GPU")
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
              "rounds": args.rounds}
    for name in args.steps:
        result[name] = STEPS[name](args, Deadline(args.limit))
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
