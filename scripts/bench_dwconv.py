#!/usr/bin/env python
"""Depthwise-conv microbenchmark on ConvNeXt-L's four stage shapes at micro-batch 64:
(64,56,56,192), (64,28,28,384), (64,14,14,768), (64,7,7,1536).

Times the three K21 depthwise kernels (mmpt_dwconv7_fwd / _bwd_input / _bwd_weight, NHWC, fp32
stream in, bf16 branch) beside what the reference's path runs for the same op on the same
machine: F.conv2d(groups=C) in bf16 channels_last and its autograd backward (input and weight
gradients timed together: autograd runs them as one convolution_backward).  Reports, per shape and
kernel, the time, the fraction of the HBM peak (8 TB/s) against the compulsory bytes — 6 B per
element forward (4-B read, 2-B write), 2 + 4 + 4 B for the input gradient, 2 + 4 B for the weight
gradient — and the ratio to torch.  HIP events, warm-up first, random N(0,1) operands.

python scripts/bench_dwconv.py [--iters 20] [--batch 64]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_llm_pretraining_amd import kernels as K  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (MI355X spec)


def timeit(fn, iters):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    torch.manual_seed(0)
    B = args.batch
    for H, C in ((56, 192), (28, 384), (14, 768), (7, 1536)):
        n = B * H * H * C
        x = torch.randn(B, H, H, C, device="cuda")
        w = (torch.randn(49, C, device="cuda") * 0.1).to(torch.bfloat16)
        bias = torch.randn(C, device="cuda").to(torch.bfloat16)
        c = torch.empty(B, H, H, C, device="cuda", dtype=torch.bfloat16)
        dc = torch.randn(B, H, H, C, device="cuda").to(torch.bfloat16)
        dx = torch.randn(B, H, H, C, device="cuda")
        dw, db = torch.zeros(49, C, device="cuda"), torch.zeros(C, device="cuda")
        t_f = timeit(lambda: K.dwconv7_fwd(x, w, bias, c), args.iters)
        t_i = timeit(lambda: K.dwconv7_bwd_input(dc, w, dx, dx_in=dx), args.iters)
        t_w = timeit(lambda: K.dwconv7_bwd_weight(x, dc, dw, db), args.iters)
        # torch: bf16 channels_last, as the reference's model runs it under autocast
        xt = x.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        xt.requires_grad_(True)
        wt = w.t().reshape(C, 1, 7, 7).contiguous().requires_grad_(True)
        bt = bias.clone().requires_grad_(True)
        gt = dc.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            tt_f = timeit(lambda: F.conv2d(xt, wt, bt, padding=3, groups=C), args.iters)
        y = F.conv2d(xt, wt, bt, padding=3, groups=C)
        tt_b = timeit(lambda: torch.autograd.grad(y, (xt, wt, bt), gt, retain_graph=True),
                      args.iters)
        print(json.dumps({
            "shape": [B, H, H, C],
            "fwd_us": round(t_f * 1e6, 1), "bwd_input_us": round(t_i * 1e6, 1),
            "bwd_weight_us": round(t_w * 1e6, 1),
            "fwd_hbm_frac": round(6 * n / t_f / HBM_PEAK, 3),
            "bwd_input_hbm_frac": round(10 * n / t_i / HBM_PEAK, 3),
            "bwd_weight_hbm_frac": round(6 * n / t_w / HBM_PEAK, 3),
            "torch_fwd_us": round(tt_f * 1e6, 1), "torch_bwd_us": round(tt_b * 1e6, 1),
            "fwd_vs_torch": round(t_f / tt_f, 3),
            "bwd_vs_torch": round((t_i + t_w) / tt_b, 3)}), flush=True)


if __name__ == "__main__":
    main()
