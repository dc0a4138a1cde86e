# Run-to-run bit stability of the library GEMMs in deterministic mode
# (DESIGN.md item 18).  In the mode every hipBLASLt plan is the heuristic's
# top-1; whether each such solution gives the same bits on every call is not
# visible from the code (the weight-grad shapes run beta = 1 into fp32, and
# stream-K solutions exist in the candidate lists), so this measures it: for
# every shape of ob_layer_lt_shapes at the benchmark workload (GPT-2 small,
# 8 x 1024) and at the 6.7B block (4096 x 32, 2 x 1024), CALLS calls on the
# same operands, counting outputs that differ from the first call's.
#
#   OB_DETERMINISTIC=1 python tools/det_probe.py [OUT.json]
#   (default profiles/det_lt_stability.json)
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from oobleck_amd._ext import (LT_SHAPE_NAMES, ObLayerDesc, check, get_ext,  # noqa: E402
                              layer_lt_shapes, lt_shape)
from oobleck_amd.config import GPT2_SMALL, GPT3_6_7B  # noqa: E402
from tests.gpu_helpers import ptr, stream  # noqa: E402

CALLS = 20
DEV = "cuda:0"
WORKLOADS = [("gpt2-small 8x1024", GPT2_SMALL, 8, 1024, (1, 2)),
             ("6.7B block 2x1024", GPT3_6_7B, 2, 1024, (1,))]


def probe(ext, s, g):
    sd = dict(zip(LT_SHAPE_NAMES, s))
    M, N, K = sd["M"], sd["N"], sd["K"]
    ab = torch.float32 if sd["ab_f32"] else torch.bfloat16
    cd = torch.float32 if sd["c_f32"] else torch.bfloat16

    def rand(rows, ld, dtype, scale):
        return (torch.randn(rows, ld, generator=g, device=DEV) * scale).to(dtype)
    A = rand(K if sd["tA"] else M, sd["lda"], ab, 0.5)
    Bm = rand(N if sd["tB"] else K, sd["ldb"], ab, 0.05)
    C0 = rand(M, sd["ldc"], cd, 1.0) if sd["beta1"] and not sd["cin"] else \
        torch.zeros(M, sd["ldc"], device=DEV, dtype=cd)
    bias = torch.randn(N, generator=g, device=DEV) if sd["bias"] else None
    res = rand(M, sd["ldc"], cd, 0.5) if sd["cin"] else None
    first, differ = None, 0
    for _ in range(CALLS):
        C = C0.clone()
        if sd["cin"]:
            rc = ext.ob_gemm_lt_bias_res(sd["tA"], sd["tB"], M, N, K, 1.0,
                                         ptr(A), sd["lda"], ptr(Bm), sd["ldb"],
                                         ptr(C), sd["ldc"], sd["c_f32"],
                                         ptr(bias), ptr(res), stream())
        elif sd["bias"]:
            rc = ext.ob_gemm_lt_bias(sd["tA"], sd["tB"], M, N, K, 1.0, ptr(A),
                                     sd["lda"], ptr(Bm), sd["ldb"],
                                     1.0 if sd["beta1"] else 0.0, ptr(C),
                                     sd["ldc"], sd["c_f32"], ptr(bias),
                                     stream())
        else:
            rc = ext.ob_gemm_lt(sd["tA"], sd["tB"], M, N, K, 1.0, ptr(A),
                                sd["lda"], ptr(Bm), sd["ldb"],
                                1.0 if sd["beta1"] else 0.0, ptr(C), sd["ldc"],
                                sd["c_f32"], stream())
        if rc < 0:
            return sd, None, None  # the library has no solution: not routed
        check(rc, "gemm_lt")
        torch.cuda.synchronize()
        if first is None:
            first = C
        elif not torch.equal(first, C):
            differ += 1
    index = ext.ob_gemm_lt_plan_index(lt_shape(*s), stream())
    return sd, differ, index


def main():
    out = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else \
        ROOT / "profiles" / "det_lt_stability.json"
    ext = get_ext()
    if not ext.ob_deterministic():
        raise SystemExit("run with OB_DETERMINISTIC=1: the probe measures the "
                         "plans the mode uses")
    g = torch.Generator(device=DEV).manual_seed(3)
    rows = []
    for wname, mc, B, S, kinds in WORKLOADS:
        for kind in kinds:
            d = ObLayerDesc(kind=kind, n_embd=mc.n_embd, n_head=mc.n_head,
                            n_positions=mc.n_positions,
                            vocab_size=mc.vocab_size, max_batch=B, seq_len=S,
                            n_slots=1, dtype=1)
            for s in layer_lt_shapes(d):
                sd, differ, index = probe(ext, s, g)
                rows.append({"workload": wname, "kind": kind, "shape": sd,
                             "solution_index": index, "calls": CALLS,
                             "differ_from_first": differ})
                print(wname, kind, sd, "index", index, "differ", differ,
                      flush=True)
    unstable = [r for r in rows if r["differ_from_first"]]
    rec = {"device": torch.cuda.get_device_name(0), "calls_per_shape": CALLS,
           "shapes": len(rows), "unstable_shapes": len(unstable),
           "keys": rows}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(f"{len(rows)} shapes, {len(unstable)} unstable -> {out}")


if __name__ == "__main__":
    main()
