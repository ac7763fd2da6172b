#!/usr/bin/env python
"""Padded batches: the unpadded (varlen) training step against the dense full-width step, at the
bench model and micro-batch.  Text lengths are drawn per sample from U{text_len/2 .. text_len}
(the variable-length dummy dataset, right-padded by `pad_collate`); the dense side runs the
fixed-length dataset at full width.  Reports the step time and tokens per second of both
(valid tokens for the padded batches) and their ratio, then the isolated attention forward /
backward (+ rope backward) times at the same geometry: the dense entries over [B, S] against
the varlen entries over the same ragged lengths.  Each side also lists its GEMM time per step
by kernel and shape (every launch bracketed by events on one extra step).

python scripts/bench_varlen.py [--model vit-b16-pythia-1b] [--micro-batch 256] [--steps 5]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodal_llm_pretraining_amd import config as C  # noqa: E402
from multimodal_llm_pretraining_amd import kernels as K  # noqa: E402
from multimodal_llm_pretraining_amd.data import (DummyMultimodalLanguageModelingDataset,  # noqa: E402
                                                 DummyTextModelingDataset, pad_collate)
from multimodal_llm_pretraining_amd.engine import rope_tables  # noqa: E402
from multimodal_llm_pretraining_amd.models import get_model_class  # noqa: E402
from multimodal_llm_pretraining_amd.optim import AdamConfig  # noqa: E402
from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig  # noqa: E402


def dataset(cfg, text_len, seed, min_text):
    if cfg.multimodal:
        v = cfg.vision
        return DummyMultimodalLanguageModelingDataset(
            vocab_size=cfg.text.n_vocab, sequence_length=text_len + v.num_patches,
            image_size=v.image, num_samples=20_000, image_token_id=cfg.image_token_id,
            image_tokens=v.num_patches, seed=seed, min_text_length=min_text)
    return DummyTextModelingDataset(cfg.text.n_vocab, text_len, num_samples=50_000, seed=seed,
                                    min_text_length=min_text)


def timeit(fn, iters, warm=3):
    for _ in range(warm):
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
    ap.add_argument("--model", default="vit-b16-pythia-1b")
    ap.add_argument("--micro-batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="attention micro-benchmark repetitions")
    args = ap.parse_args()
    cfg = C.get_config(args.model)
    mc = get_model_class("vit-b16-pythia-1b" if args.model.startswith("tiny") else args.model)
    npch = cfg.vision.num_patches if cfg.multimodal else 0
    text_len = mc.sequence_length - npch
    mbs = args.micro_batch
    tr = ManualTrainer(StepConfig(model=args.model, micro_batch_size=mbs, scheduler="constant"),
                       AdamConfig(lr=1e-5), "cuda")
    res = {"model": args.model, "micro_batch": mbs, "width": text_len + npch,
           "text_len_range": [text_len // 2, text_len]}
    lens = None
    for side, min_text in (("dense", None), ("varlen", text_len // 2)):
        ds = dataset(cfg, text_len, 1, min_text)
        batches = []
        for s in range(args.warmup + args.steps):
            samples = [ds[s * mbs + i] for i in range(mbs)]
            b = pad_collate(samples) if min_text else \
                {k: torch.stack([x[k] for x in samples]) for k in samples[0]}
            batches.append(tr.stage({k: v.pin_memory() for k, v in b.items()}))
        if min_text:
            lens = batches[-1].lens
        torch.cuda.synchronize()

        def step(i):
            return tr.train_step([batches[i]], batches[i].num_items)

        def alloc_stats():
            st = torch.cuda.memory_stats()
            return {k: st.get(k, 0) for k in ("num_alloc_retries", "num_device_alloc", "num_device_free")}

        for i in range(args.warmup):
            step(i)
        tr.flush()
        torch.cuda.synchronize()
        a0 = alloc_stats()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(args.warmup, args.warmup + args.steps):
            loss = step(i)
        tr.flush()
        e.record()
        torch.cuda.synchronize()
        sec = s.elapsed_time(e) * 1e-3
        a1 = alloc_stats()
        toks = sum(b.T for b in batches[args.warmup:])
        res[side] = {"step_ms": round(sec / args.steps * 1e3, 2), "tokens_per_step": toks // args.steps,
                     "tokens_per_s": round(toks / sec, 1),
                     "loss_last": round(loss.item() / batches[-1].num_items, 4)}
        # the caching allocator over the timed steps (every step of the padded side has another
        # T, so no activation buffer has the size of the previous step's), and the same step on
        # ONE batch repeated (constant T): the difference is what the changing sizes cost
        res[side]["allocator_over_timed_steps"] = {k: a1[k] - a0[k] for k in a0}
        last = args.warmup + args.steps - 1
        for _ in range(2):
            step(last)
        tr.flush()
        torch.cuda.synchronize()
        a0 = alloc_stats()
        s.record()
        for _ in range(args.steps):
            step(last)
        tr.flush()
        e.record()
        torch.cuda.synchronize()
        a1 = alloc_stats()
        res[side]["same_batch_repeated"] = {
            "step_ms": round(s.elapsed_time(e) / args.steps, 2), "tokens": batches[last].T,
            "tokens_per_s": round(batches[last].T * args.steps / (s.elapsed_time(e) * 1e-3), 1),
            "allocator": {k: a1[k] - a0[k] for k in a0}}
        # where the time goes: one more step with every GEMM launch bracketed by events
        K.start_gemm_probe()
        step(args.warmup + args.steps - 1)
        tr.flush()
        torch.cuda.synchronize()
        agg: dict = {}
        for name, _fl, _by, e0, e1, shp, _st in K.stop_gemm_probe():
            ent = agg.setdefault((name, tuple(shp)), [0.0, 0])
            ent[0] += e0.elapsed_time(e1)
            ent[1] += 1
        top = sorted(agg.items(), key=lambda kv: -kv[1][0])
        res[side]["gemm_ms_per_step"] = round(sum(v[0] for v in agg.values()), 1)
        res[side]["gemm_top"] = [{"kernel": k[0], "M_N_K_epi": list(k[1]), "launches": v[1],
                                  "ms": round(v[0], 1)} for k, v in top[:8]]
        del batches
        torch.cuda.empty_cache()
    res["valid_tokens_per_s_over_dense_tokens_per_s"] = round(
        res["varlen"]["tokens_per_s"] / res["dense"]["tokens_per_s"], 4)
    res["step_time_ratio_varlen_over_dense"] = round(res["varlen"]["step_ms"] / res["dense"]["step_ms"], 4)
    res["valid_token_fraction"] = round(res["varlen"]["tokens_per_step"] / res["dense"]["tokens_per_step"], 4)
    print(json.dumps(res), flush=True)

    # isolated attention at the same geometry (GPTNeoX interleaved qkv, causal)
    t = cfg.text
    H, D, S, B = t.heads, t.head_dim, text_len + npch, mbs
    hs, ps, scale = 3 * D, D, D ** -0.5
    cos, sin = (x.cuda() for x in rope_tables(t.hidden, H, t.rotary_pct, t.rope_theta, S))
    rot = cos.shape[1]
    att = {"B": B, "S": S, "H": H, "D": D}
    for side in ("dense", "varlen"):
        T = B * S if side == "dense" else sum(lens)
        qkv = torch.randn(T, 3 * H * D, device="cuda").to(torch.bfloat16)
        dout = torch.randn(T, H * D, device="cuda").to(torch.bfloat16)
        out = torch.empty(T, H * D, device="cuda", dtype=torch.bfloat16)
        dqkv = torch.empty_like(qkv)
        if side == "dense":
            lse = torch.empty(B * H * S, device="cuda")
            fwd = lambda: K.attention_fwd(qkv, B, S, H, D, hs, ps, True, scale, out, lse)  # noqa: E731
            bwd = lambda: K.attention_bwd_rope(qkv, B, S, H, D, hs, ps, True, scale, out, dout, lse,  # noqa: E731
                                               dqkv, rot, cos, sin)
        else:
            mx = max(lens)
            lse = torch.empty(B * H * mx, device="cuda")
            cu = K.cu_seqlens_of(lens).cuda()
            pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).cuda()
            fwd = lambda: K.attention_varlen_fwd(qkv, lens, cu, H, H, D, hs, ps, 2 * ps, True, scale,  # noqa: E731
                                                 out, lse, max_seq=mx)

            def bwd():
                K.attention_varlen_bwd(qkv, lens, cu, H, H, D, hs, ps, 2 * ps, True, scale, out, dout,
                                       lse, dqkv, max_seq=mx)
                K.rope_inplace(dqkv, S, H, D, rot, hs, ps, cos, sin, inverse=True, pos=pos)
        tf = timeit(fwd, args.iters)
        tb = timeit(bwd, args.iters)
        exact = 2.0 * H * D * (B * S * S if side == "dense" else sum(n * n for n in lens))
        att[side] = {"tokens": T, "fwd_us": round(tf * 1e6, 1), "bwd_rope_us": round(tb * 1e6, 1),
                     "fwd_tflops_exact": round(exact / tf / 1e12, 1),
                     "bwd_tflops_exact": round(2.5 * exact / tb / 1e12, 1)}
        del qkv, dout, out, dqkv
    print(json.dumps({"attention": att}), flush=True)


if __name__ == "__main__":
    main()
