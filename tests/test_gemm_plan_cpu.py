"""CPU-only tests of the GEMM launch schedule (csrc/gemm_plan.h).

test_queries_match_table: the five shape-only queries of the loaded library (workspace bytes,
plan, kernel name, column-sum rows, fused row-sum rows) against tests/golden/gemm_plan_table.json,
row for row.  The queries are host arithmetic: without a GPU the CU count falls back to 256, the
MI355X's own, so the table holds on both kinds of machine.

test_schedule_invariants: scripts/diag/gemm_plan_check.cpp, built with the host sanitizers, sweeps
gemm_schedule() itself.

`python tests/test_gemm_plan_cpu.py` regenerates the table (for the day a plan change is intended).

One table row per shape: {"s": [M, N, K], "cs": mmpt_gemm_colsum_rows, "acs":
mmpt_gemm_acc_colsum_rows, "e": {epilogue: [workspace bytes, tile, splits, names (workspace 0),
tile, splits, names (the queried workspace)]}} — the second triple only where the workspace is not
0.  names = "<one letter per layout pair (0,0) (0,1) (1,1) (1,0)>:<launch epilogue>": 4 =
gemm4p_kernel, K = gemm4p_kt_kernel, 1 = gemm128_kernel, - = the pair is not legal for the shape.
"""

import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "gemm_plan_table.json")
PAIRS = [(0, 0), (0, 1), (1, 1), (1, 0)]
FAMILY = {"gemm4p_kernel": "4", "gemm4p_kt_kernel": "K", "gemm128_kernel": "1"}


def shapes():
    out = []

    def linears(T, h, ffn):  # forward, input gradient, weight gradient of the four Linears
        for n, k in ((3 * h, h), (h, h), (ffn, h), (h, ffn)):
            out.extend([(T, n, k), (T, k, n), (n, k, T)])

    # DESIGN §3's table (T = 180,992; the 180,224 rows above the forward tail; ViT 50,432)
    for T in (180992, 180224):
        linears(T, 2048, 8192)
    linears(50432, 768, 3072)
    # per-rank 32 (T = 22,624, ViT 6,304 tokens), C2 (T = 32,784), C5 (Pythia-2.8B's widths)
    linears(22624, 2048, 8192)
    linears(6304, 768, 3072)
    linears(32784, 2048, 8192)
    linears(69568, 2560, 10240)
    out += [(130816, 50304, 2048), (130816, 2048, 50304), (50304, 2048, 130816)]  # lm_head
    # the GPU tests' shapes: test_gemm_tail_split, test_gemm_wgrad_tail_split,
    # test_gemm_wgrad_colsum*, test_gemm4p_k_tail_weight_gradient, test_gemm_query_names_the_launch
    out += [(m, 2048, 2048) for m in (256 * 35, 256 * 34 + 100, 256 * 32 + 16, 256 * 32 + 100)]
    out += [(5120, 3328, 8192), (5120, 3328, 8208), (3328, 5120, 8192), (3328, 5120, 8208)]
    out += [(6144, 2048, 45248), (2296, 776, 50432), (4000, 4000, 8192), (2304, 768, 50432),
            (2048, 2048, 22600), (2048, 2048, 45248), (768, 768, 50432), (2048, 10240, 8192)]
    out += [(4096, 4096, 18464), (2560, 10240, 34784), (8192, 8192, 1000)]
    out += [(512, 512, 256), (4096, 2048, 128), (2048, 4096, 1096), (4096, 4096, 1096),
            (2048, 2048, 8192)]
    # tiny: one tile, 75 / 127 / 128 tiles of 256^2
    out += [(256, 256, 256), (64, 8, 8), (3840, 1280, 1024), (127 * 256, 256, 1024),
            (4096, 2048, 1024)]
    return sorted(set(out))


def legal_epilogues(M, N, K):
    # SWIGLU pairs 128-column gate | up blocks, DSWIGLU writes them; F32_ACC_COLSUM takes K_ROWS
    # operands (contiguous dims multiples of 8)
    return [e for e in range(13)
            if not (e == 10 and N % 256) and not (e == 11 and N % 128)
            and not (e == 12 and (M % 8 or N % 8))]


def legal_pair(la, lb, epi, M, N, K):
    if epi == 12 and (la, lb) != (1, 1):
        return False
    return not ((M if la else K) % 8 or (N if lb else K) % 8)


def _lib():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from multimodal_llm_pretraining_amd import _lib as L

    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    L.load()
    return L


def query_row(L, M, N, K):
    def at(epi, ws):
        tile, splits = ctypes.c_int(0), ctypes.c_int(0)
        L.call("mmpt_gemm_plan", M, N, K, epi, ws, ctypes.byref(tile), ctypes.byref(splits))
        fam, tails = "", set()
        for la, lb in PAIRS:
            if not legal_pair(la, lb, epi, M, N, K):
                fam += "-"
                continue
            buf = ctypes.create_string_buffer(64)
            L.call("mmpt_gemm_kernel_name", la, lb, epi, M, N, K, ws, buf, 64)
            kern, args = buf.value.decode().split("<")
            a, b, e = args.rstrip(">").split(", ")
            assert (int(a), int(b)) == (la, lb), buf.value
            fam += FAMILY[kern]
            tails.add(e)
        assert len(tails) == 1, (M, N, K, epi, tails)  # one launch epilogue whatever the layouts
        return [tile.value, splits.value, f"{fam}:{tails.pop()}"]

    row = {"s": [M, N, K], "cs": L.query("mmpt_gemm_colsum_rows", M, N, K),
           "acs": L.query("mmpt_gemm_acc_colsum_rows", M, N, K), "e": {}}
    for epi in legal_epilogues(M, N, K):
        ws = L.query("mmpt_gemm_workspace_bytes", M, N, K, epi)
        row["e"][str(epi)] = [ws] + at(epi, 0) + (at(epi, ws) if ws else [])
    return row


def test_queries_match_table():
    bad_env = [k for k in os.environ if k.startswith("MMPT_GEMM_")]
    assert not bad_env, f"the table holds for the default switches; unset {bad_env}"
    L = _lib()
    table = json.load(open(TABLE))
    assert [tuple(r["s"]) for r in table] == shapes()
    diffs = []
    for want in table:
        got = query_row(L, *want["s"])
        for key in ("cs", "acs"):
            if got[key] != want[key]:
                diffs.append((want["s"], key, got[key], want[key]))
        assert sorted(got["e"]) == sorted(want["e"]), want["s"]
        for epi, w in want["e"].items():
            if got["e"][epi] != w:
                diffs.append((want["s"], "epilogue " + epi, got["e"][epi], w))
    assert not diffs, f"{len(diffs)} rows differ (shape, what, got, table): {diffs[:8]}"


def test_schedule_invariants(tmp_path):
    exe = str(tmp_path / "gemm_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "diag", "gemm_plan_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]


if __name__ == "__main__":
    rows = [query_row(_lib(), *s) for s in shapes()]
    with open(TABLE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows -> {TABLE}")
