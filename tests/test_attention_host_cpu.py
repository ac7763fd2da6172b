"""CPU-only tests of the attention host layer (csrc/attn_plan.h and the entries of attention.hip).

test_plan_invariants: scripts/diag/attn_plan_check.cpp, built with the host sanitizers, sweeps
attn_plan() itself.

test_workspace_queries: both backward workspace queries of the loaded library against the formula
of include/mmpt.h, computed here, with MMPT_ATTN_DS on and off.

test_rejections_match_table: every attention entry called with one (or two) bad arguments and
made-up pointers; the status and the mmpt_last_error() text must be those recorded in
tests/golden/attention_arg_errors.json, row for row.  Skipped where a GPU is present: a row that a
regression stopped rejecting would reach a kernel launch with made-up pointers.

`python tests/test_attention_host_cpu.py` regenerates the table (for the day a message change is
intended); it refuses to record a call that was not rejected.

One table row: [id, status, error text]; id = "<entry> <overridden arguments> <switches>".
"""

import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "attention_arg_errors.json")
ERR_ARG = -1
SWITCHES = ("MMPT_ATTN_DS", "MMPT_ATTN_PAIR", "MMPT_ATTN_NATIVE80")

# A call every entry accepts (pointers: made-up, 16-B aligned); a row overrides some of it.
BASE = dict(batch=2, seq=64, total=100, heads=4, kv_heads=2, head_dim=64, qkv=0x100000, ld=768,
            hs=64, ps=256, koff=256, voff=512, causal=1, scale=0.125, cu=0x700000, out=0x200000,
            dout=0x400000, ld_out=256, lse=0x300000, dqkv=0x500000, ws=0x600000, rot=32,
            cos=0x800000, sin=0x900000, stream=None)
# the D = 256 call mmpt_attention_bwd_rope runs fused (64 rotary dims, 16-B aligned tables)
FUSED = dict(head_dim=256, rot=64, ld=3072, hs=768)

ENTRIES = {
    "fwd": ("mmpt_attention_fwd",
            "batch seq heads head_dim qkv ld hs ps causal scale out ld_out lse stream"),
    "bwd": ("mmpt_attention_bwd",
            "batch seq heads head_dim qkv ld hs ps causal scale out dout ld_out lse dqkv ws stream"),
    "bwd_rope": ("mmpt_attention_bwd_rope",
                 "batch seq heads head_dim qkv ld hs ps causal scale out dout ld_out lse dqkv ws rot "
                 "cos sin stream"),
    "gqa_fwd": ("mmpt_attention_gqa_fwd",
                "batch seq heads kv_heads head_dim qkv ld hs koff voff causal scale out ld_out lse "
                "stream"),
    "gqa_bwd": ("mmpt_attention_gqa_bwd",
                "batch seq heads kv_heads head_dim qkv ld hs koff voff causal scale out dout ld_out "
                "lse dqkv ws stream"),
    "varlen_fwd": ("mmpt_attention_varlen_fwd",
                   "batch seq total heads kv_heads head_dim qkv ld hs koff voff causal scale cu out "
                   "ld_out lse stream"),
    "varlen_bwd": ("mmpt_attention_varlen_bwd",
                   "batch seq total heads kv_heads head_dim qkv ld hs koff voff causal scale cu out "
                   "dout ld_out lse dqkv ws stream"),
}


def rows():
    """(entry, overridden arguments, switches) of every bad call."""
    out = []

    def add(entry, sw=None, **over):
        out.append((entry, over, sw or {}))

    for e, (_, names) in ENTRIES.items():
        names = names.split()
        for d in (72, 48, 144):
            add(e, head_dim=d)
        for dim in ("batch", "seq", "heads"):
            add(e, **{dim: 0})
        add(e, qkv=0)
        add(e, qkv=0x100008)
        add(e, ld=770)
        add(e, hs=68)
        add(e, out=0)
        add(e, lse=0)
        add(e, ld_out=260)
        add(e, batch=1 << 20, seq=1 << 11)  # batch * seq = 2^31
        add(e, batch=1, seq=1 << 20, ld=1024)  # one sequence spans 2 GiB
        if "ws" in names:
            add(e, dout=0)
            add(e, dqkv=0)
            add(e, ws=0)
        if "ps" in names:  # k / v offsets = ps, 2 ps
            add(e, ps=260)
            add(e, ps=-8)
        if "koff" in names:
            add(e, kv_heads=3)
            add(e, kv_heads=0)
            add(e, koff=-8)
            add(e, koff=260)
            add(e, voff=12)
            add(e, voff=-16)
            add(e, koff=-8, kv_heads=3)  # two defects: the head count wins
            add(e, out=0, kv_heads=3)    # the entry's pointers are checked before the kv geometry
        if "cu" in names:
            add(e, seq=0, cu=0)  # max_seq wins
            add(e, seq=-1)
            add(e, cu=0)
            add(e, cu=0x700002)
            add(e, total=1)
            add(e, total=2 * 64 + 1)
            add(e, cu=0, total=1)        # cu_seqlens before total_tokens
            add(e, total=1, out=0)       # total_tokens before the entry's pointers
            add(e, head_dim=72, cu=0)    # the dense checks before the varlen ones
            add(e, batch=3, total=2)
        # two defects at once: the precedence of the shared checks
        add(e, head_dim=72, qkv=0)
        add(e, batch=0, head_dim=72)
        add(e, ld=770, out=0)
        add(e, qkv=0, lse=0)

    e = "bwd_rope"
    for over in (dict(rot=3), dict(rot=0), dict(rot=-2), dict(rot=66), dict(cos=0), dict(sin=0),
                 dict(rot=3, head_dim=72), dict(cos=0, batch=0), dict(FUSED, rot=258)):
        add(e, **over)
    # the fused arm (D = 256, 64 rotary dims, aligned tables, dS tiles + wave pairs) has its own
    # texts; with a switch off or a table off 16 B the call goes through mmpt_attention_bwd
    for sw in ({}, {"MMPT_ATTN_PAIR": 0}, {"MMPT_ATTN_DS": 0}):
        add(e, sw, dout=0, **FUSED)
        add(e, sw, ps=260, **FUSED)
        add(e, sw, heads=0, **FUSED)
        add(e, sw, head_dim=256, rot=64, ld=3076, hs=768)
    add(e, dout=0, cos=0x800004, **FUSED)
    add(e, ws=0, sin=0x900008, **FUSED)
    add(e, ps=260, cos=0x800004, **FUSED)
    add(e, ld_out=260, **dict(FUSED, rot=32))
    add(e, ps=260, dqkv=0, **FUSED)  # the part stride is a qkv stride here, checked first
    # the 80-dim path under both settings: the same rejections
    for sw in ({"MMPT_ATTN_NATIVE80": 0}, {"MMPT_ATTN_NATIVE80": 1}):
        add("gqa_fwd", sw, head_dim=80, out=0)
        add("varlen_bwd", sw, head_dim=80, ws=0)
    return out


def row_id(entry, over, sw):
    return " ".join([entry, ",".join(f"{k}={v}" for k, v in over.items()),
                     ",".join(f"{k}={v}" for k, v in sw.items())]).rstrip()


def _lib():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from multimodal_llm_pretraining_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    L.load()
    return L


def _default_switches():
    bad_env = [k for k in SWITCHES if k in os.environ]
    assert not bad_env, f"these tests hold for the default switches; unset {bad_env}"


def answer(L, entry, over, sw):
    """(status, mmpt_last_error()) of one bad call, under the row's switches."""
    symbol, names = ENTRIES[entry]
    args = dict(BASE, **over)
    prev = {}
    try:
        for k, v in sw.items():
            prev[k] = L.set_switch(k, v)
        status = L.query(symbol, *[args[n] for n in names.split()])
        return status, L.query("mmpt_last_error").decode()
    finally:
        for k, v in prev.items():
            L.set_switch(k, v)


@pytest.mark.skipif(torch.cuda.is_available(),
                    reason="bad-argument calls carry made-up pointers: never run them where a "
                           "kernel could launch (a CPU-only machine checks this table)")
def test_rejections_match_table():
    _default_switches()
    L = _lib()
    table = json.load(open(TABLE))
    want_ids = [row_id(*r) for r in rows()]
    assert len(set(want_ids)) == len(want_ids)
    assert [t[0] for t in table] == want_ids
    diffs = []
    for (rid, status, text), r in zip(table, rows()):
        assert status != 0, rid
        got = answer(L, *r)
        if got != (status, text):
            diffs.append((rid, got, (status, text)))
    assert not diffs, f"{len(diffs)} rows differ (row, got, table): {diffs[:8]}"


def test_workspace_queries():
    _default_switches()
    L = _lib()

    def delta(b, s, h):  # fp32 per query row
        return b * s * h * 4

    def with_tiles(b, s, h):  # δ 256-B rounded, then ceil(S/32)^2 tiles of 2 KiB per (batch, head)
        nq = -(-s // 32)
        return -(-delta(b, s, h) // 256) * 256 + b * h * nq * nq * 2048

    dims = [(b, s, h, d) for b, s, h in ((1, 1, 1), (2, 707, 8), (3, 31, 5), (1, 32, 7), (5, 33, 3),
                                         (8, 2048, 16), (1, 8192, 32))
            for d in (64, 80, 96, 112, 128, 256)]
    for on in (1, 0):
        prev = L.set_switch("MMPT_ATTN_DS", on)
        try:
            for b, s, h, d in dims:
                dense = with_tiles(b, s, h) if d == 256 and on else delta(b, s, h)
                assert L.query("mmpt_attention_bwd_workspace_bytes", b, s, h, d) == dense, (on, b, s, h, d)
                # varlen: δ only at every head dim, whatever the switch
                assert L.query("mmpt_attention_varlen_bwd_workspace_bytes", b, s, h, d) == \
                    delta(b, s, h), (on, b, s, h, d)
        finally:
            L.set_switch("MMPT_ATTN_DS", prev)


def test_plan_invariants(tmp_path):
    exe = str(tmp_path / "attn_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "diag", "attn_plan_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]


if __name__ == "__main__":
    assert not torch.cuda.is_available(), "record the table on a machine without a GPU"
    _default_switches()
    lib = _lib()
    table = []
    for r in rows():
        status, text = answer(lib, *r)
        assert status == ERR_ARG, f"not rejected as a bad argument ({status}, {text!r}): {row_id(*r)}"
        table.append([row_id(*r), status, text])
    with open(TABLE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(t) for t in table) + "\n]\n")
    print(f"{len(table)} rows -> {TABLE}")
