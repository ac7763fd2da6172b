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

With --packed: the four varlen kernels (mmpt_*_varlen_*) on the same operands against the dense
ones, in one process, alternated: per repeat, each kernel's dense form, its varlen form with equal
lengths (B sequences of 4096: the same work, so the difference is the cost of the position loads
and the table search) and its varlen form on a ragged cut of the same T tokens into documents of
500-4096 tokens drawn from --seed.  Reports the median over --repeats and the repeat-to-repeat
spread, (max - min) / median, of every figure.

python scripts/bench_mamba.py [--iters 10] [--batches 1,8] [--step] [--ckpt]
python scripts/bench_mamba.py --packed [--iters 10] [--repeats 5] [--batches 1,8] [--seed 0]
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


def ragged_lens(T, seed, lo=500, hi=4096):
    """T tokens cut into documents of lo..hi tokens (the last one takes what is left)."""
    g = torch.Generator().manual_seed(seed)
    lens = []
    while T > 0:
        n = min(T, int(torch.randint(lo, hi + 1, (1,), generator=g)))
        lens.append(n)
        T -= n
    return lens


def kernels(B, iters, packed=False, repeats=5, seed=0):
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
    if packed:
        scan = (u, dt, dt_bias, A_log, Bm, Cm, D, xz[:, I:])
        sbwd = scan + (dy, du, dxz[:, I:], ddt, dproj[:, R:R + N], dproj[:, R + N:], dA, dD, dbias)
        conv = (xz[:, :I], w, bias)
        cbwd = conv + (du, dxz[:, :I], dw, db)
        forms = {"dense": {
            "conv_fwd": lambda: K.causal_conv1d_fwd(*conv, u, L),
            "scan_fwd": lambda: K.selective_scan_fwd(*scan, y, L, states=states),
            "scan_bwd": lambda: K.selective_scan_bwd(*sbwd, L, states=states),
            "conv_bwd": lambda: K.causal_conv1d_bwd(*cbwd, L, du2=dy)}}

        def varlen(lens):
            tb = K.scan_tables(lens, "cuda")
            pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).cuda()
            st = K.scan_varlen_states(tb, I, N, "cuda")
            return {"conv_fwd": lambda: K.causal_conv1d_varlen_fwd(*conv, u, pos),
                    "scan_fwd": lambda: K.selective_scan_varlen_fwd(*scan, y, tb, states=st),
                    "scan_bwd": lambda: K.selective_scan_varlen_bwd(*sbwd, tb, states=st),
                    "conv_bwd": lambda: K.causal_conv1d_varlen_bwd(*cbwd, pos, du2=dy)}

        lens = ragged_lens(T, seed)
        forms["varlen_equal"], forms["varlen_ragged"] = varlen([L] * B), varlen(lens)
        order = ("conv_fwd", "scan_fwd", "scan_bwd", "conv_bwd")  # (the backwards read the forwards)
        times = {f: {k: [] for k in order} for f in forms}
        for _ in range(repeats):
            for k in order:
                for f in forms:  # alternated: the forms of one kernel run back to back
                    times[f][k].append(timeit(forms[f][k], iters))
        out = {"micro_batch": B, "tokens": T, "repeats": repeats, "ragged_documents": len(lens),
               "ragged_min_max": [min(lens), max(lens)]}
        for f in forms:
            for k in order:
                v = sorted(times[f][k])
                med = v[len(v) // 2]
                out[f"{f}_{k}_us"] = round(med * 1e6, 1)
                out[f"{f}_{k}_spread"] = round((v[-1] - v[0]) / med, 4)
        for f in ("varlen_equal", "varlen_ragged"):
            for k in order:
                out[f"{f}_{k}_vs_dense"] = round(out[f"{f}_{k}_us"] / out[f"dense_{k}_us"], 4)
        print(json.dumps(out), flush=True)
        return
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
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    torch.manual_seed(0)
    for b in (int(v) for v in args.batches.split(",")):
        if args.step:
            step(b, args.ckpt)
        else:
            kernels(b, args.iters, args.packed, args.repeats, args.seed)


if __name__ == "__main__":
    main()
