#!/usr/bin/env python
"""Mamba microbenchmark at the mamba-2.8b recipe's shape (sequences of 4096, d_inner 5120, 16
states, dt rank 160), per micro-batch.

Times the four K22 kernels (mmpt_causal_conv1d_fwd / _bwd, mmpt_selective_scan_fwd / _bwd) on the
layouts the engine gives them (x | z as halves of one [T, 2I] buffer, B and C as columns of the
x_proj output) and reports the time and the fraction of the HBM peak (8 TB/s) against the
compulsory bytes per (token, channel): conv forward 2 + 2 B, conv backward 2 + 2 + 2 read and 2
written, scan forward 3 x 2 read and 2 written, scan backward 4 x 2 read and 3 x 2 written (B, C,
the parameters and the chunk states are small beside these).  HIP events, warm-up first, random
operands.

With --step: estimate_step_time for the `mamba-2.8b` model type (one GPU, the recipe's batch of 128
reached by accumulation) at the same micro-batches, plain and with ZeRO-1 + optimizer offload, and
mfu / executed_mfu against the dense bf16 peak (2.5 PFLOP/s; the two FLOP counts are the same
number for this family).

python scripts/bench_mamba.py [--iters 10] [--batches 1,8] [--step] [--ckpt]
"""

from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_llm_pretraining_amd import config as C  # noqa: E402
from multimodal_llm_pretraining_amd import kernels as K  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (MI355X spec)
PEAK_BF16 = 2.5e15  # FLOP / s, dense bf16 MFMA


def timeit(fn, iters):
    for _ in range(2):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def kernels(B, iters):
    t = C.get_config("mamba-2.8b").text
    L, I, N, R = 4096, t.d_inner, t.d_state, t.rank
    T = B * L
    bf = torch.bfloat16
    rnd = lambda *s: torch.randn(*s, device="cuda")  # noqa: E731
    xz, proj = rnd(T, 2 * I).to(bf), rnd(T, R + 2 * N).to(bf)
    w, bias = (rnd(4, I) * 0.4).to(bf), (rnd(I) * 0.1).to(bf)
    u, dt, y = torch.empty(T, I, device="cuda", dtype=bf), (0.3 * rnd(T, I)).to(bf), \
        torch.empty(T, I, device="cuda", dtype=bf)
    dlt = torch.exp(torch.empty(I, device="cuda").uniform_(math.log(1e-3), math.log(0.1)))
    dt_bias = dlt + torch.log(-torch.expm1(-dlt))
    A_log = torch.log(torch.arange(1, N + 1, device="cuda").float()).expand(I, N).contiguous()
    D = torch.ones(I, device="cuda")
    dy, du, ddt = rnd(T, I).to(bf), torch.empty(T, I, device="cuda", dtype=bf), \
        torch.empty(T, I, device="cuda", dtype=bf)
    dxz, dproj = torch.empty_like(xz), torch.empty_like(proj)
    dw, db = torch.zeros(4, I, device="cuda"), torch.zeros(I, device="cuda")
    dA, dD, dbias = torch.zeros(I, N, device="cuda"), torch.zeros(I, device="cuda"), \
        torch.zeros(I, device="cuda")
    states = K.scan_states(B, L, I, N, "cuda")
    Bm, Cm = proj[:, R:R + N], proj[:, R + N:]
    t_cf = timeit(lambda: K.causal_conv1d_fwd(xz[:, :I], w, bias, u, L), iters)
    t_sf = timeit(lambda: K.selective_scan_fwd(u, dt, dt_bias, A_log, Bm, Cm, D, xz[:, I:], y, L,
                                               states=states), iters)
    t_sb = timeit(lambda: K.selective_scan_bwd(u, dt, dt_bias, A_log, Bm, Cm, D, xz[:, I:], dy, du,
                                               dxz[:, I:], ddt, dproj[:, R:R + N],
                                               dproj[:, R + N:], dA, dD, dbias, L, states=states),
                  iters)
    t_cb = timeit(lambda: K.causal_conv1d_bwd(xz[:, :I], w, bias, du, dxz[:, :I], dw, db, L, du2=dy),
                  iters)
    n = T * I
    out = {"micro_batch": B, "tokens": T}
    for name, sec, nbytes in (("conv_fwd", t_cf, 4), ("conv_bwd", t_cb, 8), ("scan_fwd", t_sf, 8),
                              ("scan_bwd", t_sb, 14)):
        out[name + "_us"] = round(sec * 1e6, 1)
        out[name + "_TBps"] = round(nbytes * n / sec / 1e12, 3)
        out[name + "_hbm_frac"] = round(nbytes * n / sec / HBM_PEAK, 3)
    print(json.dumps(out), flush=True)


def step(mbs, ckpt):
    from multimodal_llm_pretraining_amd.experiments import TrainingConfig, TrainingTimeEmpirical
    from multimodal_llm_pretraining_amd.models import get_model_class

    mc = get_model_class("mamba-2.8b")
    flops = C.flops_per_sample(mc.model_config, mc.sequence_length) * mc.batch_size
    for sharding, off in (("", False), ("zero_1", True)):
        cfg = TrainingConfig(1, 1, "mi355x", "mamba-2.8b", activation_checkpointing=ckpt,
                             sharding=sharding, offloading=off)
        r = TrainingTimeEmpirical(cfg, benchmarking_steps=2).run(max_micro_batch_size=mbs,
                                                                  num_samples=4 * mbs)
        st = r.get("step_time")
        print(json.dumps({"model": "mamba-2.8b", "sharding": sharding or "ddp", "offload": off,
                          "checkpointing": ckpt, "micro_batch": r.get("micro_batch_size"),
                          "step_time_s": st and round(st, 3),
                          "mfu": st and round(flops / st / PEAK_BF16, 4),
                          "executed_mfu": st and round(flops / st / PEAK_BF16, 4),
                          "training_days": r.get("training_days")}), flush=True)
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--ckpt", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    for b in (int(v) for v in args.batches.split(",")):
        if args.step:
            step(b, args.ckpt)
        else:
            kernels(b, args.iters)


if __name__ == "__main__":
    main()
