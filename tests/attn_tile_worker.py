"""Worker of tests/test_gpu_attn_routes.py::test_flash_tiling2: ONE process with USSEG_FLASH_TILE=2 in its environment (the fused
attention reads it once per process), running flash cases of the route matrix on the <2, 4> kernels.  Writes the worst err / bound
ratio of every output per case and whether all passed; exits non-zero on the first failure.

usage: USSEG_FLASH_TILE=2 python tests/attn_tile_worker.py <out.json> '<json list of [B, N, heads, out32, view]>'
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]

if __name__ == "__main__":
    assert os.environ.get("USSEG_FLASH_TILE") == "2", "run with USSEG_FLASH_TILE=2"
    from test_gpu_attn_routes import run_flash_case
    out, cases = sys.argv[1], json.loads(sys.argv[2])
    res = {"ok": False, "cases": []}
    for B, N, nh, o32, view in cases:
        ratios = run_flash_case(B, N, nh, o32, view, 2, seed=7000 + 1000 * nh + N)
        res["cases"].append({"case": [B, N, nh, o32, view], "worst": ratios})
        print(f"\n[tile 2] B{B} N{N} h{nh} o32={o32} view={view}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()), flush=True)
    res["ok"] = True
    with open(out, "w") as fh:
        json.dump(res, fh)
