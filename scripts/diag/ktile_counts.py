#!/usr/bin/env python
"""Instruction-class counts of a gemm4p kernel's K loop, from `hipcc -S` output.

usage: python scripts/diag/ktile_counts.py gemm.s KERNEL [KERNEL ...]

  cd multimodal_llm_pretraining_amd/csrc
  hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../include --cuda-device-only -S gemm.hip -o gemm.s

KERNEL is the mangled name or a part of it that picks one function, e.g.
`gemm4p_kernelILi1ELi1ELi3E`.  The K loop is the smallest loop (a label and a later branch back
to it) that holds at least 128 v_mfma; a loop over pairs of K-tiles holds 256, and the counts are
printed per K-tile (per 128 v_mfma).  Instructions are classed by mnemonic prefix only.  Prints
one JSON line per kernel, with NumVgprs / NumAgprs / ScratchSize / LDS bytes / code length."""

import json
import re
import sys

CLASSES = (  # first matching prefix wins
    ("mfma", ("v_mfma",)),
    ("lds_dma", ()),  # buffer_/global_load ... lds (set below)
    ("lds", ("ds_",)),
    ("scratch", ("scratch_",)),
    ("vmem", ("buffer_", "global_", "flat_")),
    ("waitcnt", ("s_waitcnt",)),
    ("barrier", ("s_barrier",)),
    ("branch", ("s_cbranch", "s_branch")),
    ("salu", ("s_",)),
    ("valu", ("v_",)),
)


def classify(mnemonic, operands):
    if mnemonic.startswith(("buffer_load", "global_load")) and re.search(r"\blds\b", operands):
        return "lds_dma"
    for name, prefixes in CLASSES:
        if mnemonic.startswith(prefixes) and prefixes:
            return name
    return "other"


def function_lines(lines, key):
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\S*:", l) and key in l.split(":")[0]]
    if len(starts) != 1:
        names = [lines[i].split(":")[0] for i in starts]
        raise SystemExit(f"{key!r} matches {len(starts)} functions {names[:6]}")
    s = starts[0]
    e = next(i for i in range(s, len(lines)) if lines[i].startswith(".Lfunc_end"))
    info = {}
    for l in lines[e:e + 40]:
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|NumSgprs): (\d+)", l) or \
            re.match(r"^; (codeLenInByte) = (\d+)", l) or re.match(r"^; (LDSByteSize): (\d+)", l)
        if m:
            info[m.group(1)] = int(m.group(2))
    return lines[s].split(":")[0], lines[s + 1:e], info


def k_loop(body):
    """(first, last) body indices of the smallest loop with >= 128 v_mfma."""
    label_at = {}
    insts = []  # (body index, mnemonic, operands)
    for i, l in enumerate(body):
        t = l.split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            label_at[m.group(1)] = len(insts)
            continue
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        parts = t.split(None, 1)
        insts.append((i, parts[0], parts[1] if len(parts) > 1 else ""))
    best = None
    for n, (_, mn, ops) in enumerate(insts):
        if not mn.startswith(("s_cbranch", "s_branch")):
            continue
        tgt = label_at.get(ops.strip())
        if tgt is None or tgt > n:
            continue
        loop = insts[tgt:n + 1]
        if sum(1 for _, m_, _ in loop if m_.startswith("v_mfma")) < 128:
            continue
        if best is None or len(loop) < len(best):
            best = loop
    return best


def main():
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    lines = open(sys.argv[1]).read().splitlines()
    for key in sys.argv[2:]:
        name, body, info = function_lines(lines, key)
        loop = k_loop(body)
        if loop is None:
            raise SystemExit(f"{name}: no loop with 128 v_mfma")
        counts = {}
        for _, mn, ops in loop:
            c = classify(mn, ops)
            counts[c] = counts.get(c, 0) + 1
        ktiles = counts["mfma"] / 128.0
        per = {c: round(v / ktiles, 1) for c, v in sorted(counts.items())}
        per["total"] = round(len(loop) / ktiles, 1)
        print(json.dumps({"kernel": name, "ktiles_per_loop": ktiles, "per_ktile": per, **info}))


if __name__ == "__main__":
    main()
