"""Time of one full-batch step of the linear probe (nv_probe_grad + its reduce launch + nv_probe_step) against its two floors and against the
same mathematics in stock torch fp32 on the device, the small bank, and a whole 500-step fit.

    python tools/probe_bench.py                    # device events, 5 rounds with the sides taking turns, median [min ... max]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/probe_bench.py --trace      # kernel times: a run of its own, a few steps only
    rocprofv3 --pmc FETCH_SIZE -d <dir> -- python tools/probe_bench.py --trace            # bytes fetched per launch: a run of its own

Floors, from the constants the project counts with: bytes N d 4 B / 6.3 TB/s (the bank read once); matrix time 4 N d M16 / 155 TFLOP/s with
M16 = M rounded up to the 16 columns of an MFMA tile (both products).  The torch side is handed the features standardised ONCE ahead of the
loop (what a torch user would do); the native side standardises on load in every step."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurovit_amd import FeatureBank, LinearProbe, ops  # noqa: E402

HBM, MFMA32 = 6.3e12, 155e12
BETAS, EPS = (0.9, 0.999), 1e-8


def make(N, d, C, H, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn((N, d), device="cuda", generator=g)
    X = torch.nn.functional.normalize(X, dim=1) + 0.3 / d ** 0.5
    labels = torch.randint(0, C, (N,), device="cuda", generator=g, dtype=torch.int32)
    return X, labels


class Native:
    def __init__(self, X, labels, C, H):
        N, d = X.shape
        M = H * C
        self.X, self.labels, self.C, self.H = X, labels, C, H
        st = ops.probe_stats(X)
        self.mean, self.rstd = st["mean"], st["rstd"]
        self.denom = ops.probe_stats(labels=labels, num_classes=C)["denom"]
        self.W, self.b = torch.zeros((M, d), device="cuda"), torch.zeros(M, device="cuda")
        self.dW, self.db, self.loss = torch.empty_like(self.W), torch.empty_like(self.b), torch.empty(H, device="cuda")
        self.state = [torch.zeros_like(self.W), torch.zeros_like(self.W), torch.zeros_like(self.b), torch.zeros_like(self.b)]
        self.ws = torch.empty(ops.probe_grad_workspace_bytes(N, d, M), dtype=torch.uint8, device="cuda")
        self.l2 = [10.0 ** (-4 + h % 4) for h in range(H)]
        self.k = 0

    def step(self):
        self.k += 1
        sizes, _ = ops.probe_adam_constants(self.k, [0.01] * self.H, BETAS)
        heads = ops.probe_heads(self.H, self.C, self.l2, sizes)
        ops.probe_grad(self.X, self.W, self.b, heads, self.denom, labels=self.labels, mean=self.mean, rstd=self.rstd, out=(self.dW, self.db, self.loss),
                       workspace=self.ws)
        ops.probe_step(self.W, self.b, self.dW, self.db, *self.state, heads, self.k, BETAS, EPS)


class Torch:
    """the same objective and update in stock torch fp32 ops (matmul, softmax, Adam written out), on pre-standardised features"""

    def __init__(self, nat: Native):
        self.Z = (nat.X - nat.mean) * nat.rstd
        self.y = nat.labels.long()
        self.C, self.H = nat.C, nat.H
        self.W, self.b = torch.zeros_like(nat.W), torch.zeros_like(nat.b)
        self.mW, self.vW, self.mb, self.vb = (torch.zeros_like(t) for t in (nat.W, nat.W, nat.b, nat.b))
        self.l2 = torch.tensor(nat.l2, device="cuda").repeat_interleave(nat.C)[:, None]
        self.onehot = torch.nn.functional.one_hot(self.y, nat.C).float()[:, None, :]
        self.k = 0

    def step(self):
        self.k += 1
        N = self.Z.shape[0]
        logit = torch.addmm(self.b, self.Z, self.W.T).view(N, self.H, self.C)
        lp = torch.log_softmax(logit, dim=2)
        self.loss = -(lp * self.onehot).sum(2).mean(0)
        G = ((lp.exp() - self.onehot) / N).view(N, -1)
        dW = torch.addmm(self.l2 * self.W, G.T, self.Z)
        db = G.sum(0)
        size, bc2s = 0.01 / (1 - BETAS[0] ** self.k), (1 - BETAS[1] ** self.k) ** 0.5
        for p, g, m, v in ((self.W, dW, self.mW, self.vW), (self.b, db, self.mb, self.vb)):
            m.mul_(BETAS[0]).add_(g, alpha=1 - BETAS[0])
            v.mul_(BETAS[1]).addcmul_(g, g, value=1 - BETAS[1])
            p.addcdiv_(m, v.sqrt().div_(bc2s).add_(EPS), value=-size)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # microseconds per call


def fmt(xs):
    return f"{statistics.median(xs):9.1f} [{min(xs):.1f} ... {max(xs):.1f}]"


def bench_case(N, d, C, H, rounds, iters):
    X, labels = make(N, d, C, H)
    nat = Native(X, labels, C, H)
    tor = Torch(nat)
    for side in (nat, tor):
        for _ in range(3):
            side.step()
    torch.cuda.synchronize()
    tn, tt = [], []
    for _ in range(rounds):                       # the sides take turns
        tn.append(timed(nat.step, iters))
        tt.append(timed(tor.step, iters))
    M16 = 16 * ((H * C + 15) // 16)
    bytes_us, mfma_us = N * d * 4 / HBM * 1e6, 4.0 * N * d * M16 / MFMA32 * 1e6
    agree = ((nat.W - tor.W).abs().max() / tor.W.abs().max().clamp(min=1e-30)).item()
    print(f"| {N} x {d} | C={C} H={H} (M={H * C}) | {fmt(tn)} | {fmt(tt)} | {bytes_us:.1f} | {mfma_us:.1f} | {statistics.median(tn) / max(bytes_us, mfma_us):.1f}x | "
          f"{statistics.median(tt) / statistics.median(tn):.2f}x | {agree:.1e} |", flush=True)
    del nat, tor, X
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--trace", action="store_true", help="a few native steps of 78820 x 1024, C=2 H=8, and nothing else (for a rocprofv3 run)")
    args = ap.parse_args()
    if args.trace:
        X, labels = make(78820, 1024, 2, 8)
        nat = Native(X, labels, 2, 8)
        for _ in range(5):
            nat.step()
        torch.cuda.synchronize()
        print(f"traced 5 steps; the bank holds {X.numel() * 4} bytes, the chunk workspace {nat.ws.numel()} bytes")
        return
    print(f"device: {torch.cuda.get_device_name(0)}; {args.rounds} rounds of {args.iters} steps per side, the sides taking turns; microseconds per step, median [min ... max]")
    print("| bank | heads | native step (3 launches) | torch fp32 step | byte floor | MFMA time | native / floor | torch / native | weights agree |")
    print("|---|---|---|---|---|---|---|---|---|")
    for N, d in ((78820, 1024), (78820, 768)):
        for C, H in ((2, 1), (2, 8), (5, 6)):
            bench_case(N, d, C, H, args.rounds, args.iters)
    bench_case(4096, 768, 2, 8, args.rounds, args.iters)
    # a whole fit: 500 steps, 8 heads, wall clock with one synchronisation at the end (includes the host's per-step work: two C calls)
    X, labels = make(78820, 1024, 2, 8)
    bank = FeatureBank.from_features(X, labels=labels)
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        probe = LinearProbe(1024, num_classes=2, l2=[10.0 ** (-4 + h % 4) for h in range(8)]).fit(bank, steps=500)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    hist = probe.history.cpu()
    print(f"whole fit, 78820 x 1024, C=2 H=8, 500 steps (statistics included): {statistics.median(walls):.1f} ms [{min(walls):.1f} ... {max(walls):.1f}] wall; "
          f"loss {hist[0].tolist()[0]:.4f} -> {hist[-1].min().item():.4f} .. {hist[-1].max().item():.4f}")


if __name__ == "__main__":
    main()
